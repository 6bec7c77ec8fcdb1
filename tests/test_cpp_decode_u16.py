"""The C++ host mirror's Decode / DecodeUtf16 / DecodeBatchUtf16 (include/tkz_tokenizer.hpp) compiled with g++ and run through the C ABI, on a handful of the
cases of tests/u8_decode_cases.py: on CPU against the emulated build of the kernels, on the GPU box against libtkz.so.  The expected bytes and code units are
the plain reference's, embedded in the program by this driver (decode_u16_cases.inc)."""
import gzip
import os
import subprocess

import pytest

import u16_cases as U
import u8_decode_cases as D
from conftest import GOLDEN, ROOT


def cpp_list(values):
    return "{" + ",".join(str(int(v)) for v in values) + "}"


def write_cases(path, oracle_mod, raw):
    S = U.DecodeSetup(oracle_mod.Vocab(raw).entries())
    lut = D.byte_ids(S)
    hand = [U.DecodeCase("hand_" + h.replace(" ", ""), lut[list(bytes.fromhex(h))], [0, len(bytes.fromhex(h))]) for h, _ in D.HAND]
    mixed = U.DecodeCase("specials_strays_and_a_cut_char", [S.max_id + 1, int(lut[0xF0]), int(lut[0x9F]), S.strays[0], int(lut[0x98]), int(lut[0x80]), S.max_id + 20,
                                                         S.known[5], int(lut[0xE4]), int(lut[0xB8]), int(lut[0xAD])], [0, 0, 6, 10, 11])
    cases = hand + [mixed] + D.split_char_cases(S)[:3] + D.ragged_tail_cases(S)[5:7] + D.unit_extreme_cases(S)[1:] + \
        [D.sweep_case(S, D.PROBES[2], 1, "boundary", D.sweep_edges(D.WORD)), D.sweep_case(S, D.PROBES[6], 2, "inside", D.sweep_edges(D.WORD))]
    lines = ["static const tkz::SpecialTokens kSpecials = {%s};" % ", ".join('{"%s", %d}' % (k, v) for k, v in S.specials.items()),
             "static const std::vector<Case> kCases = {"]
    for case in cases:
        docs = D.documents(S, case)
        batches = [case.ids[int(a):int(b)] for a, b in zip(case.offs, case.offs[1:])]
        lines.append('  {"%s", {%s},\n   {%s},\n   {%s}},' % (case.name, ",".join(cpp_list(b) for b in batches), ",".join(cpp_list(d) for d in docs),
                                                            ",".join(cpp_list(D.get_string(d)) for d in docs)))
    lines.append("};")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(cases)


def build_and_run(tmp_path, oracle_mod, libdir, libname):
    raw = gzip.decompress(open(os.path.join(GOLDEN, "gpt2.tiktoken.gz"), "rb").read())
    vocab = tmp_path / "gpt2.tiktoken"
    vocab.write_bytes(raw)
    n = write_cases(str(tmp_path / "decode_u16_cases.inc"), oracle_mod, raw)
    exe = str(tmp_path / "test_decode_u16")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), "-I", str(tmp_path), os.path.join(ROOT, "tests", "cpp", "test_decode_u16.cpp"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe, str(vocab)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cpp decode mirror ok: %d cases" % n in out.stdout


def test_cpp_decode_mirror_on_emulated_kernels(tmp_path, oracle_mod):
    import emu
    emu.library()
    build_and_run(tmp_path, oracle_mod, os.path.dirname(emu.EMU_LIB), "tkz_hostemu")


@pytest.mark.gpu
def test_cpp_decode_mirror_on_gpu(tmp_path, oracle_mod):
    build_and_run(tmp_path, oracle_mod, os.path.join(ROOT, "tokenizer_amd", "lib"), "tkz")
