"""MI355X-native engine for CellRegMap's per-variant score-test path.

Exports the names of the reference package (cellregmap/__init__.py:1-20).
"""
from enum import Enum

from ._engine import (
    CellRegMap,
    GenotypePanel,
    candidate_groups,
    detect_groups,
    compute_maf,
    estimate_betas,
    estimate_betas_many,
    get_L_values,
    lrt_pvalues,
    predict_interaction_many,
    release_workspaces,
    run_association,
    run_association_fast,
    run_association_many,
    run_interaction,
    run_interaction_contexts,
    run_interaction_contexts_joint,
    run_interaction_contexts_joint_many,
    run_interaction_contexts_many,
    run_interaction_many,
    scan_association_many,
    scan_interaction_contexts_joint_many,
    scan_interaction_contexts_many,
    scan_interaction_many,
    scan_interaction_resumable,
)


class Term(Enum):
    """cellregmap/_types.py:1-8."""

    FIXED = 1
    RANDOM = 2


__version__ = "0.6.0"

__all__ = [
    "__version__",
    "CellRegMap",
    "GenotypePanel",
    "candidate_groups",
    "detect_groups",
    "run_association",
    "run_association_fast",
    "run_association_many",
    "run_interaction",
    "run_interaction_contexts",
    "run_interaction_contexts_joint",
    "run_interaction_contexts_joint_many",
    "run_interaction_contexts_many",
    "run_interaction_many",
    "scan_association_many",
    "scan_interaction_contexts_joint_many",
    "scan_interaction_contexts_many",
    "scan_interaction_many",
    "scan_interaction_resumable",
    "compute_maf",
    "estimate_betas",
    "estimate_betas_many",
    "get_L_values",
    "lrt_pvalues",
    "predict_interaction_many",
    "release_workspaces",
    "Term",
]
