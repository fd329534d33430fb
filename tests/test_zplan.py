"""The z-chunk plan of every stage and pair launch (porousfreezethaw_amd/csrc/pft_zplan.h) on the CPU:
tests/native/zplan_check.cpp, a stand-alone program over that header alone, enumerates slabs, tile
counts, occupancies, CU counts, forced and automatic kz, every range code and both boundary depths,
walks every workgroup of every plan through the decode the kernels use, and checks that each plane
of the requested range is run exactly once, that the leading workgroups of the inline placements
hold the exchanged planes, and that the cost model gives the values of the loop it was moved from.
Built with AddressSanitizer and UBSan."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "zplan_check.cpp")


def test_every_plan_tiles_its_range_under_sanitizers(tmp_path):
    exe = tmp_path / "zplan_check_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    plans, workgroups = map(int, p.stdout.split())
    # (the enumeration did run: some 10^4 plans, 10^7 workgroups)
    assert plans > 50_000 and workgroups > 10_000_000
