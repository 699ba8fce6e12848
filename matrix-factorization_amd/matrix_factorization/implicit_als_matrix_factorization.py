"""ImplicitALSMF: implicit-feedback matrix factorisation by confidence-weighted
alternating least squares (Hu, Koren & Volinsky 2008).

The reference has no implicit-feedback model (its interaction table carries a
``rating/implicit`` column that can only go through the explicit SGD).  Here
``y`` is an interaction strength r_ui >= 0 (clicks, plays, counts):

    confidence  c_ui = 1 + alpha r_ui,   preference  p_ui = [r_ui > 0]
    every pair that is not in X:         c = 1, p = 0
    L = sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + reg (sum_u |x_u|^2 + sum_i |y_i|^2)

over ALL n_users x n_items pairs, no biases, no global mean.  With the items
fixed and G = Y^T Y,

    (G + sum_{i in I_u} alpha r_ui y_i y_i^T + reg I) x_u
        = sum_{i in I_u, r_ui > 0} (1 + alpha r_ui) y_i

and the same for the items with the roles swapped.  A user without
observations keeps its row; one whose strengths are all 0 gets the zero vector.
One epoch = users, then items, then the loss.

``solver="direct"`` (the default) solves each of these k x k systems exactly;
``solver="cg"`` takes ``cg_steps`` conjugate-gradient steps on it instead,
started from the entity's current row (Takacs, Pilaszy & Tikk 2011): O(k^2) a
step against the O(k^3) elimination, and the error a few steps leave is taken
up by the next epoch's warm start.  The one visible difference besides the
inexactness: with "cg" an entity whose strengths are all 0 moves towards the
zero vector by those steps, it is not set to it.

Everything around fit --
RNG draw order of the initial factors, predict, recommend, recommend_batch,
pickling -- is KernelMF's (linear kernel, float32 parameters, zero biases, so a
score is exactly x_u . y_i).
"""

from __future__ import annotations

import numpy as np
import pandas as pd

from .engine import ImplicitALS
from .kernel_matrix_factorization import KernelMF


class ImplicitALSMF(KernelMF):
    """Implicit-feedback factor model fitted by ALS on the GPU (mf_gramian +
    mf_ials_sweep: f32-input MFMA Gramians + LDS elimination per entity, or
    mf_ials_sweep_cg: the same Gramians + conjugate gradients in LDS).

    Arguments: n_factors (1..128), n_epochs, alpha (>= 0: confidence per unit
    of strength), reg (> 0), init_mean, init_sd, min_rating, max_rating,
    verbose, device, solver ("direct" | "cg"), cg_steps (1..1024, used by
    "cg").  After fit, ``train_loss`` lists the loss per epoch.
    """

    SOLVERS = ("direct", "cg")
    MAX_CG_STEPS = 1024

    def __init__(self, n_factors: int = 100, n_epochs: int = 15, alpha: float = 40.0,
                 reg: float = 1, init_mean: float = 0, init_sd: float = 0.1,
                 min_rating: int = 0, max_rating: int = 1, verbose: int = 1, device=None,
                 solver: str = "direct", cg_steps: int = 3):
        super().__init__(n_factors=n_factors, n_epochs=n_epochs, kernel="linear",
                         reg=reg, init_mean=init_mean, init_sd=init_sd,
                         min_rating=min_rating, max_rating=max_rating, verbose=verbose,
                         dtype="float32", schedule="exact", device=device)
        self.alpha = alpha
        self.solver = solver
        self.cg_steps = cg_steps
        self._check_hyper()

    def __setstate__(self, state):
        # pickles written before the solver choice existed: the exact solve
        for key, default in (("solver", "direct"), ("cg_steps", 3)):
            state.setdefault(key, default)
        super().__setstate__(state)

    def _check_hyper(self) -> None:
        if not np.isfinite(self.alpha) or self.alpha < 0:
            raise ValueError(f"alpha must be finite and >= 0, got {self.alpha}")
        if not np.isfinite(self.reg) or self.reg <= 0:
            raise ValueError(f"reg must be finite and > 0, got {self.reg}")
        if self.solver not in self.SOLVERS:
            raise ValueError(f"solver must be one of {self.SOLVERS}, got {self.solver!r}")
        c = self.cg_steps
        if (isinstance(c, bool) or not isinstance(c, (int, np.integer))
                or not 1 <= c <= self.MAX_CG_STEPS):
            raise ValueError(f"cg_steps must be an integer in [1, {self.MAX_CG_STEPS}], got {c!r}")

    def _check_strengths(self, y) -> None:
        v = np.asarray(y, dtype=np.float64)
        if not np.all(np.isfinite(v)) or np.any(v < 0):
            raise ValueError("interaction strengths must be finite and >= 0")

    def _run(self, eng, n_epochs: int, users_only: bool, verbose: int) -> list:
        als = ImplicitALS(eng)
        cg = int(self.cg_steps) if self.solver == "cg" else None
        pending, loss = [], []
        for epoch in range(n_epochs):
            als.sweep_users(self.alpha, self.reg, cg)
            if not users_only:
                als.sweep_items(self.alpha, self.reg, cg)
            pending.append(als.loss_async(self.alpha, self.reg))
            if verbose == 1:
                loss.append(float(pending[-1].item()))
                print("Epoch ", epoch + 1, "/", n_epochs, " -  train_loss:", loss[-1])
        if verbose != 1:
            loss = [float(t.item()) for t in pending]
        return loss

    def _engine(self, X: pd.DataFrame):
        eng = self._make_engine(X, len(self.user_features), len(self.item_features))
        eng.load_params(self.user_features, self.item_features,
                        self.user_biases, self.item_biases)
        return eng

    def fit(self, X: pd.DataFrame, y: pd.Series):
        """Validation first (no RNG draw on a ValueError), then ALSMF.fit's
        order: _preprocess_data (sample), normal(P), normal(Q), n_epochs
        epochs."""
        self._check_hyper()
        self._check_strengths(y)
        X = self._preprocess_data(X=X, y=y, type="fit")
        self.global_mean = 0.0
        self.user_biases = np.zeros(self.n_users)
        self.item_biases = np.zeros(self.n_items)
        self.user_features = np.random.normal(self.init_mean, self.init_sd,
                                              (self.n_users, self.n_factors))
        self.item_features = np.random.normal(self.init_mean, self.init_sd,
                                              (self.n_items, self.n_factors))
        eng = self._engine(X)
        self.train_loss = self._run(eng, self.n_epochs, False, self.verbose)
        self._sync_params(eng)
        self._pred_engine = eng
        return self

    def update_users(self, X: pd.DataFrame, y: pd.Series, n_epochs: int = 1,
                     verbose: int = 0):
        """Fold-in with the items frozen: ALSMF.update_users' bookkeeping (known
        users re-initialised, new users appended, same RNG order), then the
        user half-sweep on the given data.  With ``solver="direct"`` that is
        the exact minimiser, so further epochs repeat it; with ``solver="cg"``
        the re-initialised / new rows are the CG start, and every further
        epoch takes ``cg_steps`` more steps from the last result."""
        self._check_hyper()
        self._check_strengths(y)
        X, known_users, new_users = self._preprocess_data(X=X, y=y, type="update")
        for user in known_users:
            user_index = self.user_id_map[user]
            self.user_biases[user_index] = 0
            self.user_features[user_index, :] = np.random.normal(
                self.init_mean, self.init_sd, (1, self.n_factors))
        self.user_biases = np.append(self.user_biases, np.zeros(len(new_users)))
        new_user_features = np.random.normal(self.init_mean, self.init_sd,
                                             (len(new_users), self.n_factors))
        self.user_features = np.concatenate((self.user_features, new_user_features), axis=0)
        # n_users is not updated (KernelMF.update_users' quirk): the engine
        # takes the row counts of the arrays
        eng = self._engine(X)
        self.train_loss = self._run(eng, n_epochs, True, verbose)
        self._sync_params(eng)
        self._pred_engine = eng
