"""The C++ host mirror's pair-rows method (include/tkz_tokenizer.hpp -> tkz_encode_batch_pairs_utf8 / _utf16), compiled with g++ and run through the C ABI as
tests/test_cpp_padded.py does it: on CPU against the emulated build of the kernels, on the GPU against libtkz.so.  And tests/cpp/sanitize_pairs.cpp: a
stand-alone program, compiled here with the product sources and the CPU emulator under -fsanitize=address,undefined and run as a process of its own -- nothing
of it is loaded into this interpreter."""
import gzip
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tokenizer_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "hostemu")


def _vocab(tmp_path):
    vocab = tmp_path / "gpt2.tiktoken"
    vocab.write_bytes(gzip.decompress(open(os.path.join(GOLDEN, "gpt2.tiktoken.gz"), "rb").read()))
    return str(vocab)


def _build_and_run(tmp_path, libdir, libname):
    exe = str(tmp_path / "test_pairs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_pairs.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe, _vocab(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "cpp pairs ok" in out.stdout, out.stdout + out.stderr


def test_cpp_pairs_on_emulated_kernels(tmp_path):
    import emu
    emu.library()
    _build_and_run(tmp_path, os.path.dirname(emu.EMU_LIB), "tkz_hostemu")


@pytest.mark.gpu
def test_cpp_pairs_on_gpu(tmp_path):
    _build_and_run(tmp_path, os.path.join(ROOT, "tokenizer_amd", "lib"), "tkz")


def test_sanitized_program_on_emulated_kernels(tmp_path):
    """tests/hostemu/Makefile's source list and flags with the sanitizers added, linked into one program with its own main (the sources compile side by side)"""
    exe = str(tmp_path / "sanitize_pairs")
    sources = [os.path.join(SRC, f) for f in ("tkz_kernels.hip", "tkz_api.cpp", "tkz_vocab.cpp", "tkz_shard.cpp", "tkz_comm.cpp", "tkz_sdma.cpp")]
    sources += [os.path.join(EMU, "hip_emu.cpp"), os.path.join(ROOT, "tests", "cpp", "sanitize_pairs.cpp")]
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-attributes", "-DTKZ_HOSTEMU", "-fsanitize=address,undefined",
             "-fno-omit-frame-pointer", "-I", EMU, "-I", SRC, "-I", os.path.join(ROOT, "include")]
    objects = [str(tmp_path / (os.path.basename(src) + ".o")) for src in sources]
    jobs = [subprocess.Popen(["g++"] + flags + ["-x", "c++", "-c", src, "-o", obj]) for src, obj in zip(sources, objects)]
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    subprocess.check_call(["g++", "-fsanitize=address,undefined"] + objects + ["-ldl", "-pthread", "-o", exe])
    out = subprocess.run([exe, _vocab(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "sanitize pairs ok" in out.stdout, out.stdout[-2000:] + out.stderr[-6000:]
    assert "AddressSanitizer" not in out.stderr and "LeakSanitizer" not in out.stderr, out.stderr[-6000:]
    # UBSan: nothing in the pair kernels (tkz_kernels.hip from their banner to the budgeted section's), the entries' file or this program.  (What it reports
    # elsewhere -- left shifts of -1 in the pre-tokenizer's row masks -- is older than this feature and not this test's.)
    text = open(os.path.join(SRC, "tkz_kernels.hip")).read()
    first = text[:text.index("// Pair rows (tkz_encode_batch_pairs_device")].count("\n") + 1
    last = text[:text.index("// Token-budget buckets (tkz_encode_batch_budgeted_device")].count("\n") + 1
    for line in out.stderr.splitlines():
        if "runtime error" not in line:
            continue
        where = line.split(": runtime error")[0].split(":")
        name, row = os.path.basename(where[0]), int(where[1])
        assert name not in ("sanitize_pairs.cpp", "tkz_api.cpp") and not (name == "tkz_kernels.hip" and first <= row < last), line
