"""The persistent stream-K grid planner (boda-1_amd/csrc/bh_skgrid.h) on the CPU: a stand-alone program
(tests/skgrid/skgrid_check.cc) built with AddressSanitizer + UBSan asserts the grids the ring, direct and
Winograd launchers planned before they shared it, and the planner's invariants over a sweep; the header is
host-only, so none of it needs a GPU or the kernel library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "skgrid", "skgrid_check.cc")
INC = os.path.join(ROOT, "boda-1_amd", "csrc")
CASES = ["rows", "invariants", "knob"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("skgrid") / "skgrid_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + INC, "-o", exe, SRC],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=86", UBSAN_OPTIONS="halt_on_error=1:exitcode=87")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    return p


def test_no_sanitizer_report_and_all_pass(report):
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-3000:]
    assert "AddressSanitizer" not in report.stderr and "runtime error:" not in report.stderr
    assert "skgrid check ok" in report.stdout and "FAILED" not in report.stdout


@pytest.mark.parametrize("case", CASES)
def test_case(report, case):
    assert "case %s ok" % case in report.stdout.splitlines(), report.stdout[-2000:]
