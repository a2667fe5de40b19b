"""The chunk plan of a packed compare call (csrc/avk_pack_chunks.h) on the CPU: tests/native/pack_chunks_check.cpp, a program of its own, built with the address and
undefined-behaviour sanitizers and run — the groups' segments tile every array exactly once, stay in bounds and keep the floor; every 256-region block is run by
exactly one launch, the first one behind which its region range and its calls have arrived."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_tiles_the_arrays_and_every_block_has_one_launch(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tests/native/pack_chunks_check.cpp")
    exe = str(tmp_path / "pack_chunks_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "pack_chunks_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "pack_chunks_check: ok" in out.stdout
