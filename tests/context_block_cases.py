"""The cohorts of tests/test_gpu_context_blocks.py (plain helper module, not a test): the constructions of
tests/context_lrt_cases.py and tests/context_joint_cases.py at enough variants to span several blocks of 128, with the held
variants fixed by index on both sides of every block and sub-range boundary.  The simulator's phenotype depends on the
variant count, so these are cohorts of their own; tests/test_context_blocks_cpu.py holds every one of them, at every held
index, to the conditions the GPU tests rely on.

name -> (variants, held variants, both calls or the joint one only)

    k 3, c 9        300: blocks of 128 + 128 + 44; with room for 50 variants' rotated candidates sub-ranges of 50, 50, 28 and 44
    k 17, c 70      140: 2 176 Khatri-Rao rows in a full block; the null fit of 71 columns
    k 5, rank 260   140: the widest spectrum
    k 33, c 35      130: two candidate groups, the null on an interior grid point
    k 48, c 128     130: V in the variant's global scratch row, rows per sub-range
    dosages         140: the k 3, c 9 cohort with the panel replaced by allele counts 0/1/2 per donor, as
                    ``GenotypePanel.from_dosages(D, donor_of_cell, standardize=False)`` takes them
"""
import numpy as np

import context_joint_cases as jc

DOSAGES = "dosages, k 3, c 9, mode B"
CASES = {
    "k 3, c 9, mode B": (300, [0, 49, 50, 127, 128, 177, 178, 255, 256, 299], "both"),
    "k 17, c 70, mode B": (140, [0, 127, 128, 139], "both"),
    "k 5, rank 260, mode B": (140, [0, 127, 128, 139], "both"),
    "k 33, c 35, mode B": (130, [0, 127, 128, 129], "joint"),
    "k 48, c 128, mode B": (130, [0, 127, 128, 129], "joint"),
    DOSAGES: (140, [0, 127, 128, 139], "both"),
}
BOTH = [name for name in CASES if CASES[name][2] == "both"]
BLOCK = 128        # variants per block the GPU tests set
SUB = 50           # variants whose rotated candidates the budget of the GPU tests has room for


class DosageCase(jc.JointCase):
    """The k 3, c 9 cohort at 140 variants with the panel replaced: ``D`` (donors x 140, int8 allele counts, none
    monomorphic) and ``G`` = D expanded to cells."""

    def __init__(self, name=DOSAGES, seed=401):
        super().__init__("k 3, c 9, mode B", variants=CASES[name][0])
        self.name = name
        self.D = np.random.default_rng(seed).integers(0, 3, size=(self.donors, CASES[name][0])).astype(np.int8)
        assert np.all(self.D.min(axis=0) < self.D.max(axis=0))
        self.G = self.D[self.donor_of_cell].astype(float)


_cases = {}


def case(name):
    """One object per cohort and process."""
    if name not in _cases:
        _cases[name] = DosageCase(name) if name == DOSAGES else jc.JointCase(name, variants=CASES[name][0])
    return _cases[name]


def held(name):
    return list(CASES[name][1])
