"""The C++ host mirror's count methods (include/tkz_tokenizer.hpp -> tkz_count_utf8 / _utf16, tkz_count_batch_utf8 / _utf16), compiled with g++ and run through
the C ABI as tests/test_cpp_small_decode.py does it: on CPU against the emulated build of the kernels, on the GPU against libtkz.so."""
import gzip
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT


def _build_and_run(tmp_path, libdir, libname):
    vocab = tmp_path / "gpt2.tiktoken"
    vocab.write_bytes(gzip.decompress(open(os.path.join(GOLDEN, "gpt2.tiktoken.gz"), "rb").read()))
    exe = str(tmp_path / "test_count")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_count.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe, str(vocab)], capture_output=True, text=True)
    assert out.returncode == 0 and "cpp count ok" in out.stdout, out.stdout + out.stderr


def test_cpp_count_on_emulated_kernels(tmp_path):
    import emu
    emu.library()
    _build_and_run(tmp_path, os.path.dirname(emu.EMU_LIB), "tkz_hostemu")


@pytest.mark.gpu
def test_cpp_count_on_gpu(tmp_path):
    _build_and_run(tmp_path, os.path.join(ROOT, "tokenizer_amd", "lib"), "tkz")
