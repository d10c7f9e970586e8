"""captured.LpBudget: the one copy of the CG launch-budget formula and of the decay-and-restore rule that EpisodeGraphs and
BatchGraph each used to spell out.  Host arithmetic only: no library, no GPU."""
import pytest

from r3dfsseg_amd.captured import LpBudget


@pytest.mark.parametrize("mx", [0, 1, 10, 11, 16, 23, 37, 59, 200])
def test_budget_for(mx):
    assert LpBudget.budget_for(mx) == max(24, 8 * ((mx + mx // 2 + 8 + 7) // 8))


# (bad, mx) of consecutive finished runs -> the decaying maximum and the budget after each, worked out by hand from the
# rule: a miss keeps max(d, mx) and restores the captured maximum; otherwise d = max(mx, d - max(1, d // 16)) and the
# budget is budget_for(d); mx == 0 (nothing ran) changes nothing; every budget is clamped to [1, captured].
SCRIPT_120 = [
    # bad, mx,   d, budget
    (0, 37, 37, 64),    # d = max(37, 0 - 1); 37 + 18 + 15 = 70 -> 64
    (0, 20, 35, 64),    # 37 - max(1, 2) = 35; 35 + 17 + 15 = 67 -> 64
    (0, 20, 33, 64),    # 35 - 2 = 33; 33 + 16 + 15 = 64 -> 64
    (0, 20, 31, 56),    # 33 - 2 = 31; 31 + 15 + 15 = 61 -> 56
    (0, 0, 31, None),   # nothing ran: as before
    (3, 59, 59, 120),   # a miss: everything that was captured; d = max(31, 59)
    (0, 10, 56, 96),    # 59 - max(1, 3) = 56; 56 + 28 + 15 = 99 -> 96
    (1, 5, 56, 120),    # a miss with a small maximum keeps d
    (0, 200, 200, 120),  # 200 + 100 + 15 = 315 -> 312, clamped to the 120 captured
    (0, 1, 188, 120),   # 200 - 12 = 188; 188 + 94 + 15 = 297 -> 296, clamped
]


def test_decay_and_restore_rule():
    b = LpBudget(120)
    assert b.captured == 120 and b.active == 120
    for step, (bad, mx, d, want) in enumerate(SCRIPT_120):
        got = b.target(bad, mx)
        want = b.active if want is None else want
        assert (b._mx_decay, got) == (d, want), (step, b._mx_decay, got)
        b.active = got  # (what apply() records once the graphs are edited)


def test_small_capture_and_fixed_budget():
    b = LpBudget(16)  # fewer iterations captured than the formula's floor of 24
    assert b.target(0, 3) == 16 and b._mx_decay == 3
    b = LpBudget(120)
    b.active = 40
    assert b.target(0, 30, adaptive=False) == 40 and b._mx_decay == 0  # a fixed budget does not follow the counts ...
    assert b.target(2, 30, adaptive=False) == 120 and b._mx_decay == 30  # ... but a miss still restores everything
