"""CPU checks behind tests/test_gpu_context_blocks.py: every cohort of tests/context_block_cases.py meets, at every held
variant, the conditions the GPU tests rely on -- with the float64 oracle's own fits and the rows of
tests/test_context_lrt_reference_cpu.py and tests/test_context_joint_reference_cpu.py, the held list in place of
``pinned_reference.pick``:

  * every fitted delta -- the gene-level null's and each variant's refit under [W, C, g] -- lies in (1e-3, 1 - 1e-3);
  * 32 x the oracle's error against the longdouble reference stays below the 1e-11 ceiling, for the per-context tests and
    for the joint one, so the ceiling never sets a limit;
  * the candidates g o C_j of every held variant are well conditioned (``candidate_condition`` below 100).

Measured when the cohorts were written (null rho; gene delta; refit deltas; 32 x the oracle's worst error; worst condition):
    k 3, c 9 (300)        0.0  0.302  0.301 .. 0.418  5.0e-13   2.3
    k 17, c 70 (140)      0.0  0.788  0.799 .. 0.843  3.4e-13   7.4
    k 5, rank 260 (140)   1.0  0.949  0.939 .. 0.948  7.9e-13   2.5
    k 33, c 35 (130)      0.3  0.751  0.755 .. 0.770  4.9e-13   8.5
    k 48, c 128 (130)     0.0  0.319  0.323 .. 0.445  2.9e-13  31
    dosages, k 3 (140)    0.0  0.534  0.536 .. 0.585  2.9e-12   1.9
"""
import pytest

import context_block_cases as bc
import context_joint_cases as jc
import pinned_reference as pr
from test_context_joint_reference_cpu import _oracle_rows as _joint_rows
from test_context_lrt_reference_cpu import _oracle_rows as _each_rows


def test_the_held_variants_sit_on_both_sides_of_every_boundary():
    for name, (variants, sel, _) in bc.CASES.items():
        assert sel == sorted(set(sel)) and sel[0] == 0 and sel[-1] == variants - 1, name
        assert variants > bc.BLOCK and {bc.BLOCK - 1, bc.BLOCK} <= set(sel), name
    variants, sel, _ = bc.CASES["k 3, c 9, mode B"]
    edges = {b + s for b in range(0, variants, bc.BLOCK) for s in range(0, min(bc.BLOCK, variants - b), bc.SUB)} - {0}
    assert edges == {50, 100, 128, 178, 228, 256}
    for e in (50, 128, 178, 256):          # the first variant of a sub-range and the last of the one before it
        assert {e - 1, e} <= set(sel), e


@pytest.mark.parametrize("name", list(bc.CASES))
def test_the_block_cohorts_meet_the_conditions(name):
    cs, sel = bc.case(name), bc.held(name)
    assert cs.G.shape == (cs.n, bc.CASES[name][0])
    rho, delta0, rows = _joint_rows(cs, sel)
    worst = {"joint " + k: v for k, v in pr.worst([r[1] for r in rows]).items()}
    deltas = [r[0] for r in rows]
    if bc.CASES[name][2] == "both":
        rho_each, each = _each_rows(cs.y, cs.W, cs.C, cs.G, cs.half, cs.grid, sel)
        assert rho_each == rho
        assert [d for d, _ in each] == deltas          # (the same fits of [W, C, g])
        worst.update({"each " + k: v for k, v in pr.worst([e for _, e in each]).items()})
    cond = {j: jc.candidate_condition(cs, j) for j in sel}
    print("%s (%d cells, %d variants, held %s): rho %.1f, gene delta %.3f, refit deltas %.3f .. %.3f, "
          "32 x the oracle's error %.1e (%s), candidate condition %.1f"
          % (name, cs.n, cs.G.shape[1], sel, rho, delta0, min(deltas), max(deltas), pr.PATHS * max(worst.values()),
             ", ".join("%s %.1e" % (k, pr.PATHS * v) for k, v in sorted(worst.items())), max(cond.values())))
    assert 1e-3 < delta0 < 1 - 1e-3, (name, delta0)
    for j, delta in zip(sel, deltas):
        assert 1e-3 < delta < 1 - 1e-3, (name, j, delta)
    for key, v in worst.items():
        assert pr.PATHS * v <= pr.CEILING, (name, key, v)      # the ceiling never sets a limit
    for j in sel:
        assert cond[j] < 100.0, (name, j, cond[j])
