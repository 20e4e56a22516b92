"""The decode-lane bookkeeping (genie_tts_amd/csrc/lanes.h) is host code without HIP calls:
tools/lane_book_check.cpp drives it through the bench's call sequence, the async-generate test's
(misses, a synchronous generate in between), error re-runs and growth, against a model of the
slots.  Built here with the host AddressSanitizer + UBSan and run as a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lane_book_under_host_sanitizers(tmp_path):
    # the sanitizer runtimes linked statically (clang's default; g++ needs the flags), so the
    # program runs as it is wherever it is started
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cands = [(os.path.join(rocm, "llvm", "bin", "clang++"), []), (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), []),
             (shutil.which("clang++"), []), (shutil.which("g++"), ["-static-libasan", "-static-libubsan"])]
    cxx, extra = next(((c, x) for c, x in cands if c and os.path.exists(c)), (None, None))
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "lane_book_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *extra,
           os.path.join(ROOT, "tools", "lane_book_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "lane book ok" in r.stdout
