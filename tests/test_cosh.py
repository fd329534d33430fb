"""calc_mode 2's cosh on the device is libpft's restatement of the host C library's algorithm
(porousfreezethaw_amd/csrc/pft_cosh.h: e_cosh.c over expm1 and the table-driven exp with its fused
operations), so that mode 2 is the reference bit for bit.  Here the restatement, compiled for the
CPU without contraction, is compared (a) with committed known answers of x86-64 glibc's cosh,
which hold on any host, and (b) with the running C library on 10^7 arguments; once more under
AddressSanitizer and UBSan; and the committed table with its regeneration by mpmath."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "cosh_check.c")
FLAGS = ["-std=c99", "-ffp-contract=off", "-fno-fast-math"]


def _run(exe, n, extra):
    subprocess.run(["gcc"] + extra + FLAGS + [SRC, "-o", str(exe), "-lm"], check=True)
    p = subprocess.run([str(exe), str(n)], check=True, capture_output=True, text=True)
    print(p.stderr)
    return list(map(int, p.stdout.split()))


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("cosh") / "cosh_check", 10_000_000, ["-O2"])


def test_known_answers(counts):
    """(a) the five results that separate the FMA build of exp from the unfused one, the special
    values and both neighbours of every boundary of e_cosh.c"""
    assert counts[1] == 0, f"pft_cosh misses {counts[1]} of the committed known answers"


def test_restated_cosh_equals_c_library(counts):
    """(b) 10^7 arguments: uniform on +-25, +-2, [0, 0.7], [0, 720], [-300, 0], [709.7, 710.6],
    log-uniform down to 2^-70, random bit patterns"""
    n, _, bad_known_libm, bad = counts
    if bad_known_libm:
        pytest.skip(f"this host's cosh misses {bad_known_libm} of the known answers: its libm has no FMA variant "
                    "of exp, so it is not the C library pft_cosh restates")
    assert n == 10_000_000
    assert bad == 0, f"{bad} cosh results differ from the C library's"


def test_under_address_and_ub_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: no report, same counts"""
    n, bad_known, bad_known_libm, bad = _run(tmp_path / "cosh_check_asan", 1_000_000,
                                             ["-O1", "-g", "-fsanitize=address,undefined",
                                              "-fno-sanitize-recover=undefined"])
    assert (n, bad_known) == (1_000_000, 0)
    assert bad_known_libm or bad == 0


def test_table_regenerates():
    """the 128 committed entries equal 2^(k/128) split as scripts/gen_exp_table.py derives it"""
    pytest.importorskip("mpmath")
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "gen_exp_table.py"), "--check"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
