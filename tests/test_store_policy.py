"""The store-form policy of large long-frame updates (netflow_amd/csrc/nfcs_store_policy.h)
as a pure function of its observation history: tests/cpp/store_policy_test.cpp, a stand-alone C++ program
over the header alone (no device, no runtime), built and run here; once more as a stand-alone executable
with AddressSanitizer and UBSan. It covers the start state, the two low observations needed before sparse,
one high observation sending the context back, stale generations ignored, and alternating low and high
observations never going sparse (and the generation wrap, reset and clamping)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "store_policy_test.cpp")
INC = os.path.join(ROOT, "netflow_amd", "csrc")


def build_and_run(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra, "-I" + INC, SRC, "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "store_policy_test: ok" in r.stdout


def test_store_policy(tmp_path):
    build_and_run(tmp_path, "store_policy_test", [])


def test_store_policy_sanitized(tmp_path):
    build_and_run(tmp_path, "store_policy_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
