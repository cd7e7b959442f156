"""The explicit-GRM solve of the drivers that take ``grm_mat=`` (SKAT, SKAT-O, the conditional scan) as one record."""
from __future__ import annotations

import dataclasses
from typing import Any

import numpy as np

from . import _lib

NO_DOSAGE_KMAT = "{} with 'grm_mat' on dosage input is not implemented."


@dataclasses.dataclass(frozen=True)
class KmatSolve:
    """``Sigma = tau[0] diag(1/w) + tau[1] mat`` and the PCG limits of a solve on it: ``mat`` and ``w``, the model's weights
    V, for the scan's samples in the scan's order (``skat.aligned_grm_mat``); ``tau`` the scan model's."""
    mat: Any
    w: np.ndarray
    tau: np.ndarray
    maxiter: int
    tol: float

    def operator(self, sc):
        """The operator on ``mat``, to enter: the scanner's ``grm_operator`` (the tests' stand-ins), else the device's."""
        make = getattr(sc, "grm_operator", None)
        return _lib.ExplicitGrmOperator(self.mat) if make is None else make(self.mat)

    @property
    def args(self):
        """The trailing arguments of ``skat_kmat`` and ``cond_kmat_set`` (a scanner's and a dosage block's)."""
        return self.w, self.tau, self.maxiter, self.tol
