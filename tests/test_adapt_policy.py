"""The promotion / adaptation policy (tokenizer_amd/csrc/tkz_adapt.h) and the choice of what to promote (tkz_promo_select.h), compiled with
plain g++ and driven by tests/cpp/test_adapt_policy.cpp: no kernel, no emulator library, the production thresholds."""
import os
import subprocess

from conftest import ROOT


def test_adapt_policy(tmp_path):
    csrc = os.path.join(ROOT, "tokenizer_amd", "csrc")
    # the policy stands alone: standard headers only
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", "-include", os.path.join(csrc, "tkz_adapt.h"), os.devnull])
    exe = str(tmp_path / "test_adapt_policy")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-DTKZ_HOSTEMU", "-I", os.path.join(ROOT, "tests", "hostemu"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cpp", "test_adapt_policy.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("TKZ_ADAPT_")}
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "adapt policy ok" in out.stdout
