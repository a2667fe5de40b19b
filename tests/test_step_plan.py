"""The step plans (csrc/avk_step_plan.h) on the CPU: tests/native/step_plan_check.cpp, a program of its own, built with the address and undefined-behaviour sanitizers,
prints the chain -> slot table for every queue count; here: below eight queues every chain has one slot of at most four with the caller's chain on slot 0, from eight
queues on the plan is the identity, and an unreadable count (0, negative) is the identity too."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLER = 0


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler for tests/native/step_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("step_plan") / "step_plan_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "step_plan_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "step_plan_check: ok" in out.stdout
    plans, parsed, n_chains = {}, {}, None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[:1] == ["chains"]:
            n_chains = int(w[1])
        elif w[:1] == ["queues"]:
            plans[(int(w[1]), int(w[3]))] = (int(w[5]), [int(x) for x in w[7:]])
        elif w[:1] == ["parse"]:
            parsed[w[1].strip("'")] = int(w[-1])
    return n_chains, plans, parsed


def test_eight_chains(printed):
    n_chains, plans, _ = printed
    assert n_chains == 8  # caller, LDS solo, not wide, class C, two-call, one-call, three-call, heads' hand-backs
    assert all(len(slots) == n_chains for _, slots in plans.values())


@pytest.mark.parametrize("queues", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("lanes", [0, 1])
def test_below_eight_queues_the_chains_fold_onto_four_slots(printed, queues, lanes):
    n_chains, plans, _ = printed
    n_slots, slots = plans[(queues, lanes)]
    assert len(slots) == n_chains  # every chain has exactly one slot
    assert all(0 <= s < 4 for s in slots) and len(set(slots)) <= 4 and n_slots == 4
    assert slots[CALLER] == 0
    assert (n_slots, slots) == plans[(4, lanes)]  # one folded plan, whatever the count below eight


def test_a_step_without_lanes_has_a_stream_per_remaining_chain(printed):
    _, plans, _ = printed
    _, slots = plans[(4, 0)]
    assert sorted(slots[:4]) == [0, 1, 2, 3]  # caller, LDS solo, not wide, class C


@pytest.mark.parametrize("queues", [8, 9, 16, 24, 32, 40])
@pytest.mark.parametrize("lanes", [0, 1])
def test_from_eight_queues_on_the_plan_is_the_identity(printed, queues, lanes):
    n_chains, plans, _ = printed
    assert plans[(queues, lanes)] == (n_chains, list(range(n_chains)))


@pytest.mark.parametrize("queues", [0, -1])
def test_an_unreadable_count_selects_the_identity(printed, queues):
    n_chains, plans, _ = printed
    assert plans[(queues, 1)] == (n_chains, list(range(n_chains)))


def test_trial_plans_are_eight_digits_below_four_with_the_caller_on_slot_0(printed):
    _, _, parsed = printed
    assert parsed == {"03302012": 1, "00000000": 1, "01230123": 1, "13302012": 0, "0330201": 0, "033020123": 0, "04302012": 0, "0330201x": 0, "": 0, "null": 0}
