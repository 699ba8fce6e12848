"""BPRMF: matrix factorisation for implicit feedback by Bayesian personalised
ranking (Rendle, Freudenthaler, Gantner & Schmidt-Thieme 2009).

The reference has no ranking model.  Here ``y`` is an interaction strength
r_ui >= 0 as for ImplicitALSMF: the pairs with r > 0 are the positives, an
observed pair with r = 0 counts as unobserved.  The score is

    s(u, i) = x_u . y_i + b_i

(no user bias, no global mean), and one SGD step takes a triple (u, i, j) --
i a positive of u, j an item u has no positive for -- one step up the gradient
of  ln sigmoid(s(u,i) - s(u,j)) - reg/2 (|x_u|^2 + |y_i|^2 + |y_j|^2 + b_i^2 +
b_j^2)  (include/mf_hip.h, "BPR", states the update and its expression order).

One epoch visits every positive once in ``np.random.shuffle`` order, then draws
one 64-bit seed from the global RandomState; the negative of the triple at
visit position t is a pure function of (seed, t) computed on the GPU, rejected
against the user's positives up to 16 times (a user who holds nearly every
item has its triples skipped).  The triples are applied in conflict-free
levels that equal the sequential sweep in visit order exactly (DESIGN.md
section 4.2): no update races, the same bits whatever the launch geometry.

Everything around fit -- RNG draw order of the initial factors, predict,
recommend, recommend_batch, rank_items, evaluate_topk, pickling -- is
KernelMF's with the linear kernel, zero user biases and global mean 0.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

from .engine import BPR
from .kernel_matrix_factorization import KernelMF


class BPRMF(KernelMF):
    """BPR factor model fitted by exact-order SGD on the GPU (mf_bpr_sample,
    mf_sched_levels3, mf_bpr_epoch).

    Arguments: n_factors, n_epochs, lr (> 0), reg (>= 0), init_mean, init_sd,
    dtype ("float32" | "float64"), verbose, device.  After fit, ``train_loss``
    (mean of softplus(-z) over the epoch's triples, z taken before each
    update) and ``train_auc`` (their share with z > 0) hold one value per
    epoch.
    """

    def __init__(self, n_factors: int = 100, n_epochs: int = 20, lr: float = 0.05,
                 reg: float = 0.01, init_mean: float = 0, init_sd: float = 0.1,
                 dtype: str = "float32", verbose: int = 1, device=None):
        super().__init__(n_factors=n_factors, n_epochs=n_epochs, kernel="linear",
                         reg=reg, lr=lr, init_mean=init_mean, init_sd=init_sd,
                         min_rating=0, max_rating=1, verbose=verbose, dtype=dtype,
                         schedule="exact", device=device)
        self._check_hyper()

    def _check_hyper(self) -> None:
        if not np.isfinite(self.lr) or self.lr <= 0:
            raise ValueError(f"lr must be finite and > 0, got {self.lr}")
        if not np.isfinite(self.reg) or self.reg < 0:
            raise ValueError(f"reg must be finite and >= 0, got {self.reg}")

    def _check_strengths(self, y) -> None:
        v = np.asarray(y, dtype=np.float64)
        if not np.all(np.isfinite(v)) or np.any(v < 0):
            raise ValueError("interaction strengths must be finite and >= 0")

    def _run(self, eng, n_epochs: int, users_only: bool, verbose: int) -> None:
        bpr = BPR(eng)
        pending, loss, auc = [], [], []
        for epoch in range(n_epochs):
            pending.append(bpr.epoch(self.lr, self.reg, True, not users_only))
            if verbose == 1:
                loss.append(float(pending[-1][0].item()))
                auc.append(float(pending[-1][1].item()))
                print("Epoch ", epoch + 1, "/", n_epochs, " -  train_loss:", loss[-1],
                      " train_auc:", auc[-1])
        if verbose != 1:
            loss = [float(t[0].item()) for t in pending]
            auc = [float(t[1].item()) for t in pending]
        self.train_loss, self.train_auc = loss, auc

    def _engine(self, X: pd.DataFrame):
        eng = self._make_engine(X, len(self.user_features), len(self.item_features))
        eng.load_params(self.user_features, self.item_features,
                        self.user_biases, self.item_biases)
        return eng

    def fit(self, X: pd.DataFrame, y: pd.Series):
        """Validation first (no RNG draw on a ValueError), then
        ImplicitALSMF.fit's order: _preprocess_data (sample), normal(P),
        normal(Q); then per epoch the shuffle and the seed."""
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
        self._run(eng, self.n_epochs, False, self.verbose)
        self._sync_params(eng)
        self._pred_engine = eng
        return self

    def predict(self, X: pd.DataFrame, bound_ratings: bool = False) -> list:
        """KernelMF.predict; the scores are not ratings, so they are not
        clipped unless asked."""
        return super().predict(X, bound_ratings=bound_ratings)

    def update_users(self, X: pd.DataFrame, y: pd.Series, n_epochs: int = 20,
                     verbose: int = 0):
        """Fold-in with the items frozen: ALSMF.update_users' bookkeeping (known
        users re-initialised, new users appended, same RNG order), then
        ``n_epochs`` BPR epochs on the given data that move the user rows only
        (levels by user alone).  Negatives are rejected against the positives
        of the given data."""
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
        self._run(eng, n_epochs, True, verbose)
        self._sync_params(eng)
        self._pred_engine = eng
