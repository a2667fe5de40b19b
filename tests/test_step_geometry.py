"""The step's arithmetic (csrc/avk_step_geometry.h) on the CPU: tests/native/step_geometry_check.cpp, a program of its own, built with the address and
undefined-behaviour sanitizers, sweeps CUs x records outside the lanes x lanes on/off x slice bytes x budget x side records x class C records and checks at every
point that the four shares of the workspace (main, solo, side, early hand-backs) are pairwise disjoint and inside ws_need, that the side launch takes at most half
of the solo share and leaves the solo launch a workgroup, and that the slices stay within the budget except through the floor of eight workgroups per share.
Here: the program's verdict, the named points, and the lane geometry against bytes computed by hand."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tests/native/step_geometry_check.cpp")
    exe = str(tmp_path_factory.mktemp("step_geometry") / "step_geometry_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "step_geometry_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = out.stdout.splitlines()
    print("\n".join(l for l in lines if not l.startswith("floor")))
    assert out.returncode == 0 and "step_geometry_check: ok" in out.stdout, [l for l in lines if l.startswith("FAIL")][:20]
    return lines


def fields(line):
    w = line.split()
    return {w[i]: w[i + 1] for i in range(0, len(w) - 1) if w[i] in ("cus", "rest", "lanes", "ws", "budget", "solo_opt", "main", "solo", "early", "need", "over", "lds", "grid")}


def test_every_point_of_the_grid_passed(printed):
    assert not [l for l in printed if l.startswith("FAIL")]
    w = next(l for l in printed if l.startswith("points")).split()
    # 2 CUs x 7 sizes x 2 x 5 slice sizes x 3 budgets x 2 solo options = 840 geometries, each with 3 x 5 class C / side sizes for both side launches
    assert int(w[1]) == 840 * 3 * 5 * 2
    assert 0 < int(w[3]) < 840


def test_the_budget_is_exceeded_only_through_the_floor_of_eight(printed):
    floors = [fields(l) for l in printed if l.startswith("floor")]
    over = [f for f in floors if f["over"] == "1"]
    assert over  # the grid reaches the case: 64 MB slices under 1 GiB
    for f in over:
        assert min(int(f["main"]), int(f["solo"]), int(f["early"])) <= 8
        assert int(f["need"]) > int(f["budget"])
    for f in floors:
        if f["over"] == "0":
            assert int(f["need"]) <= int(f["budget"])


def test_the_point_of_the_small_slice_shares_test(printed):
    """tests/test_gpu_wide.py::test_small_slice_shares_do_not_overlap, 256 CUs and 1 GiB.  With 960 workgroups (768 + 128 + 64) of 4 x 4,000,000 bytes the factor is
    2^30 / 15.36e9 = 0.0699: the main launch keeps 53 workgroups, the other two the floor of eight.  With the options as that test sets them and the context's shares
    of 64 + 64 (slices of 4 << 20): 2^30 / (896 x 2^24) = 1 / 14, main 54; beside lane launches (192 + 64 + 64): 1 / 5, main 38 and 12 each."""
    pins = {l.split()[1]: fields(l) for l in printed if l.startswith("pin")}
    assert pins["decimal_4mb_128"] == {"main": "53", "solo": "8", "early": "8"}
    assert pins["binary_4mb_64"] == {"main": "54", "solo": "8", "early": "8"}
    assert pins["binary_4mb_64_lanes"] == {"main": "38", "solo": "12", "early": "12"}
    # ... and the sweep holds them: 256 CUs, slices of 4 MB, 1 GiB
    assert any(l.startswith("floor cus 256 rest 1000000 lanes 0 ws 4000000 budget 1073741824 solo_opt 0 : main 53 solo 8 early 8") for l in printed)
    assert any(l.startswith("floor cus 256 rest 1000000 lanes 0 ws 4194304 budget 1073741824 solo_opt 64 : main 54 solo 8 early 8") for l in printed)


# rows = (2 nm - 1)(W + 1) + (3 or 4 (quad) + 2 pool) x 4 (ed_max 6; 1 for ed_max 0) + qcap + 4 (nm 2) or 8; bytes = rows x 4 x width + 1152
#   class 0: W 7 nm 2 qcap 4      24 + 12 + 4 + 4 = 44        quad 24 + 16 + 8 = 48
#   class 1: W 12 nm 2 qcap 4     39 + 12 + 8 = 59            quad 63
#   class 2: W 10 nm 4 qcap 16    77 + 12 + 16 + 8 = 113      quad 117
#   class 3: W 12 nm 4 qcap 16    91 + 36 = 127               quad 131
#   class 4: W 12 nm 8 qcap 32, pool 6   195 + 60 + 40 = 295  quad 195 + 64 + 40 = 299
#   class 5: W 12 nm 2 ed_max 0   39 + 3 + 4 = 46             quad 47
LDS_BY_HAND = {(0, 64): 44 * 256 + 1152, (0, 16): 48 * 64 + 1152, (1, 64): 59 * 256 + 1152, (1, 16): 63 * 64 + 1152, (2, 64): 113 * 256 + 1152, (2, 16): 117 * 64 + 1152,
               (3, 64): 127 * 256 + 1152, (3, 16): 131 * 64 + 1152, (4, 64): 295 * 256 + 1152, (4, 16): 299 * 64 + 1152, (5, 64): 46 * 256 + 1152, (5, 16): 47 * 64 + 1152}


@pytest.mark.parametrize("cls,width", sorted(LDS_BY_HAND))
def test_lane_lds_bytes_and_grid(printed, cls, width):
    f = fields(next(l for l in printed if l.startswith("lane class %d width %d " % (cls, width))))
    lds = LDS_BY_HAND[(cls, width)]
    assert int(f["lds"]) == lds
    assert int(f["grid"]) == 256 * min(160 * 1024 // lds, 12)  # 256 CUs, at most twelve one-wave workgroups on each, 100,000 tiles to claim


def test_lane_grid_caps(printed):
    one = {" ".join(l.split()[:2]): l.split()[-1] for l in printed if l.startswith("lane ") and not l.startswith("lane class")}
    assert one == {"lane three_cap": "256",  # lane_waves_three 1: one workgroup per CU
                   "lane few_tiles": "20",   # five tiles of sixteen-record claims: no more workgroups than claims
                   "lane too_big": "0"}      # 727 rows x 256 bytes do not fit 160 KB


def test_width_log2(printed):
    got = {int(l.split()[1]): int(l.split()[2]) for l in printed if l.startswith("log2")}
    assert got == {-1: 0, 0: 0, 1: 0, 2: 1, 3: 2, 4: 2, 5: 3, 8: 3, 9: 4, 16: 4, 17: 5, 32: 5, 33: 6, 64: 6, 65: 6}
