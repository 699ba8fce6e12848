"""ContentBasedRecommender on MI355X: the reference's content-based model
(content_based.py:15-223) and two scorings that put its profiles to use.

With the internal ids of ``_preprocess_data`` and the d feature columns of
``item_features`` (every column but ``item_id``):

    F       n_items x d, FP64: row i is the first row of the frame whose item_id
            maps to internal item i (the reference takes ``.values[0]``, :125);
            rows with an unknown id are dropped (:64-65); an item without a row
            has has_features[i] = False and a zero row
    P_u     the profile of user u: with w = rating - min_rating over the user's
            training pairs whose item has features, sum w F_i / sum w when
            sum w > 0, else the undivided sum, zeros without such a pair
            (:104-134)
    S[a,b]  F_a . F_b / (|F_a| |F_b|), 0 where either norm is 0, the diagonal
            included: sklearn's ``cosine_similarity`` of the feature rows (:148)

The profiles (mf_content_profiles, FP64), the normalised rows
(mf_content_normalize, fl32(x / |x|)) and the similarity
(mf_content_similarity, float32 on the f32-input MFMA) are built on the GPU.
``scoring`` chooses what a (user, item) pair scores:

``"reference"`` (default)
    mean(P_u) for a known pair, the global mean for an unknown user or item and
    when d = 0: the reference's ``predict`` (:150-223), whose comment calls it
    a simplification.  The score does not depend on the item; ``recommend``
    works through the base class as in the reference, and ``recommend_batch``
    / ``rank_items`` / ``evaluate_topk`` raise a ValueError that names the
    other two scorings.
``"cosine"``
    cos(P_u, F_i): the dot product of the float32 rows fl32(P_u / |P_u|) and
    fl32(F_i / |F_i|) (a zero row where the norm is 0), computed by the factor
    models' mf_predict with the linear kernel, dtype float32, zero biases and
    global mean 0 -- it is that value bit for bit -- and ranked by mf_topk /
    mf_rank (ranking.RankingMixin).  The scale is the cosine's, not a rating's:
    pass ``bound_ratings=False``.  An unknown id scores 0.  d is padded with
    zero columns to a multiple of 4 (the MFMA candidate filter then serves
    d <= 64).
``"neighbors"``
    ItemItemCF's prediction with the feature similarity in place of the rating
    similarity: m_e + sum S[e,b] (r_bo - m_b) / sum |S[e,b]| over the
    ``n_neighbors`` most similar items the user rated above 0, by the
    neighbourhood models' kernels (mf_cf_predict / mf_cf_topk / mf_cf_rank)
    unchanged.

Without ``item_features``, ``fit(X, y)`` sets each profile to the user's own
mean rating and ``predict`` returns it (scoring "reference" only).

Four deliberate departures from the reference:

1. Ratings stay aligned to their pairs.  The reference's ``fit`` shuffles X in
   ``_preprocess_data`` and then assigns ``y.values`` positionally (:50-51), so
   it trains on ratings permuted against their pairs, as its neighbourhood
   models do.  Here the ratings are the ones given for each pair.
2. Without features, the reference looks external user ids up in an index of
   internal ids (:82-87), so every profile is the global mean unless the two id
   spaces happen to collide.  Here each profile is the user's own mean rating.
3. ``item_similarity_matrix`` is n_items x n_items float32 in internal-id
   order, with zero rows for items without features; the reference's is FP64
   in the frame's row order, duplicate rows included.  It is built in ``fit``
   for "neighbors" and on the first read of the attribute otherwise, and
   refused beyond ``max_similarity_bytes`` either way, as the neighbourhood
   models refuse theirs.
4. Non-numeric or non-finite feature values raise ValueError in ``fit``.
"""

from __future__ import annotations

import numpy as np
import pandas as pd
import torch

from . import _lib
from .collaborative_filtering import _UserQueries, _warn_if_no_device
from .device_model import DeviceModel, _VOID, _tp, resolve_device
from .neighbours import DEFAULT_MAX_SIMILARITY_BYTES, NeighbourEngine, check_similarity_bytes
from .ranking import RankingMixin
from .recommender_base import RecommenderBase

SCORINGS = ("reference", "cosine", "neighbors")


class ContentEngine:
    """The feature rows on one GPU and the three content-based builds."""

    def __init__(self, F: np.ndarray, has_features: np.ndarray, device=None):
        self.dev = resolve_device(device)
        self.n_items, self.d = (int(x) for x in F.shape)
        with torch.cuda.device(self.dev):
            self.F = torch.from_numpy(np.ascontiguousarray(F, np.float64)).to(self.dev)
            self.has = torch.from_numpy(np.ascontiguousarray(has_features, np.uint8)).to(self.dev)

    @property
    def stream(self):
        return _VOID(torch.cuda.current_stream(self.dev).cuda_stream)

    def profiles(self, users: np.ndarray, items: np.ndarray, weights: np.ndarray,
                 n_users: int) -> torch.Tensor:
        """FP64 n_users x d profile rows (mf_content_profiles) of the pairs
        (users[p], items[p]) with weight weights[p]; each user's list keeps the
        order of the pairs."""
        users = np.asarray(users, np.int64)
        order = np.argsort(users, kind="stable")
        ptr = np.zeros(n_users + 1, np.int64)
        np.cumsum(np.bincount(users, minlength=n_users), out=ptr[1:])
        out = torch.empty((n_users, self.d), dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.dev)  # noqa: E731
            d_ptr = to(ptr, np.int64)
            d_it = to(np.asarray(items)[order], np.int32)
            d_w = to(np.asarray(weights)[order], np.float64)
            _lib.call("mf_content_profiles", _tp(d_ptr), _tp(d_it), _tp(d_w), _tp(self.F),
                      _tp(self.has), int(n_users), self.n_items, self.d, _lib.MF_F64, _tp(out),
                      self.stream)
        return out

    def normalize(self, rows: torch.Tensor, stride: int = 0) -> torch.Tensor:
        """float32 rows fl32(x / |x|) of the FP64 device rows (mf_content_normalize),
        ``stride`` (0: d) floats apart, zero-padded."""
        n, d = (int(x) for x in rows.shape)
        out = torch.empty((n, stride or d), dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.call("mf_content_normalize", _tp(rows), n, d, int(stride), _lib.MF_F64, _tp(out),
                      self.stream)
        return out

    def similarity(self, rows: torch.Tensor) -> torch.Tensor:
        """float32 n x n products of the float32 device rows (mf_content_similarity)."""
        n, d = (int(x) for x in rows.shape)
        S = torch.empty((n, n), dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.call("mf_content_similarity", _tp(rows), n, d, _lib.MF_F32, _tp(S), self.stream)
        return S


class ContentBasedRecommender(RankingMixin, RecommenderBase):
    """Content-based filtering (content_based.py:15-223): a user's profile is
    the rating-weighted mean of the feature rows of the items they rated.

    Arguments (reference defaults): min_rating=0, max_rating=5, verbose=0; plus
    scoring ("reference" | "cosine" | "neighbors", module docstring),
    n_neighbors (default 50, "neighbors" only), device and
    max_similarity_bytes (default 16 GiB: an n_items x n_items float32
    similarity larger than this is refused with a ValueError naming the size,
    before anything is allocated).

    Attributes after fit: item_features (the mapped, filtered frame),
    user_profiles (dict: internal user id -> FP64 row, built when read),
    user_profile_matrix (n_users x d, FP64), item_similarity_matrix (float32,
    internal-id order), global_mean.
    """

    def __init__(self, min_rating: float = 0, max_rating: float = 5, verbose: int = 0,
                 scoring: str = "reference", n_neighbors: int = 50, device=None,
                 max_similarity_bytes: int = DEFAULT_MAX_SIMILARITY_BYTES):
        super().__init__(min_rating=min_rating, max_rating=max_rating, verbose=verbose)
        self.scoring = scoring
        self.n_neighbors = n_neighbors
        self.device = device
        self.max_similarity_bytes = max_similarity_bytes

    # ------------------------------------------------------------ state
    _DEVICE_STATE = ("_content", "_cosine", "_neighbour", "_S_dev")

    def __getstate__(self):
        # NumPy and builtins only; the engines are rebuilt on first use
        state = self.__dict__.copy()
        for key in self._DEVICE_STATE + ("_maps_pending", "_defer_maps"):
            state.pop(key, None)
        return state

    def __setstate__(self, state):
        for key, default in (("device", None), ("scoring", "reference"), ("n_neighbors", 50),
                             ("max_similarity_bytes", DEFAULT_MAX_SIMILARITY_BYTES)):
            state.setdefault(key, default)
        self.__dict__.update(state)
        _warn_if_no_device(type(self).__name__)

    def _fitted(self) -> None:
        if self.__dict__.get("_profiles") is None:
            raise AttributeError(f"{type(self).__name__} is not fitted")

    def _content_engine(self) -> ContentEngine:
        eng = self.__dict__.get("_content")
        if eng is None:
            if self.__dict__.get("_F") is None:
                self._fitted()
                raise ValueError("fit() was given no item_features")
            eng = self._content = ContentEngine(self._F, self._has, self.device)
        return eng

    def _similarity_device(self) -> torch.Tensor:
        S = self.__dict__.get("_S_dev")
        if S is None:
            check_similarity_bytes(self.n_items, int(self.max_similarity_bytes), "items")
            eng = self._content_engine()
            S = self._S_dev = eng.similarity(eng.normalize(eng.F))
        return S

    def _cosine_engine(self) -> DeviceModel:
        """A factor model whose rows are the normalised profiles and feature
        rows."""
        eng = self.__dict__.get("_cosine")
        if eng is None:
            ce = self._content_engine()
            dpad = (ce.d + 3) // 4 * 4
            with torch.cuda.device(ce.dev):
                P = torch.from_numpy(np.ascontiguousarray(self._profiles)).to(ce.dev)
                Pn, Qn = ce.normalize(P, dpad), ce.normalize(ce.F, dpad)
            eng = DeviceModel(self.n_users, self.n_items, dpad, "linear", "float32", self.device,
                              min_rating=self.min_rating, max_rating=self.max_rating,
                              global_mean=0.0)
            eng.load_params(Pn, Qn, np.zeros(self.n_users), np.zeros(self.n_items))
            self._cosine = eng
        return eng

    def _neighbour_engine(self) -> NeighbourEngine:
        eng = self.__dict__.get("_neighbour")
        if eng is None:
            S = self._similarity_device()
            eng = NeighbourEngine(self._train_items, self._train_users, self._train_ratings,
                                  self.n_items, self.n_users, self.device,
                                  int(self.max_similarity_bytes), what="items", similarity=S)
            self._neighbour = eng
        return eng

    def _ranking_backend(self):
        self._fitted()
        if self.scoring == "cosine":
            return self._cosine_engine()
        if self.scoring == "neighbors":
            return _UserQueries(self._neighbour_engine(), _lib.MF_CF_QUERY_OTHER,
                                int(self.n_neighbors), float(self.global_mean))
        raise ValueError(
            'scoring="reference" gives every item of a user the same score (the mean of the '
            'user\'s profile): recommend_batch, rank_items and evaluate_topk need '
            'scoring="cosine" or scoring="neighbors"')

    # -------------------------------------------------------------- API
    @staticmethod
    def _feature_values(item_features: pd.DataFrame):
        """(feature column names, FP64 values) of the frame, checked."""
        if "item_id" not in item_features.columns:
            raise ValueError("item_features must contain 'item_id' column")
        cols = [c for c in item_features.columns if c != "item_id"]
        try:
            vals = item_features[cols].to_numpy(dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"item_features columns must be numeric: {e}") from e
        vals = np.ascontiguousarray(vals).reshape(len(item_features), len(cols))
        if not np.isfinite(vals).all():
            raise ValueError("item_features holds non-finite values (NaN or inf)")
        return cols, vals

    def fit(self, X: pd.DataFrame, y: pd.Series, item_features: pd.DataFrame = None):
        """content_based.py:39-70: ``_preprocess_data`` (the reference's one RNG
        draw, id maps and duplicate check), the global mean, then the profiles
        (and for "neighbors" the similarity) on the GPU."""
        if self.scoring not in SCORINGS:
            raise ValueError(f"Unknown scoring: {self.scoring!r} (one of {SCORINGS})")
        nn = self.n_neighbors
        if isinstance(nn, bool) or not isinstance(nn, (int, np.integer)) or nn < 1:
            raise ValueError(f"n_neighbors must be an integer >= 1, got {nn!r}")
        cols = vals = None
        if item_features is not None:
            cols, vals = self._feature_values(item_features)
            kmax = _lib.load().mf_max_factors()
            if len(cols) > kmax:
                raise ValueError(f"item_features has d = {len(cols)} feature columns; at most "
                                 f"mf_max_factors() = {kmax} are supported")
        elif self.scoring != "reference":
            raise ValueError(f'scoring="{self.scoring}" needs item_features')
        X = self._preprocess_data(X=X, y=y, type="fit")
        self.global_mean = X["rating"].mean()
        for key in self._DEVICE_STATE + ("_profiles",):
            self.__dict__.pop(key, None)
        self._train_users = X["user_id"].to_numpy(np.int32)
        self._train_items = X["item_id"].to_numpy(np.int32)
        self._train_ratings = X["rating"].to_numpy(np.float64)
        self._feature_cols = cols
        if item_features is None:
            # departure 2: the user's own mean rating
            cnt = np.bincount(self._train_users, minlength=self.n_users)
            tot = np.bincount(self._train_users, weights=self._train_ratings,
                              minlength=self.n_users)
            self._F = self._has = self._feat_ids = self._feat_values = None
            self._profiles = (tot / np.maximum(cnt, 1)).reshape(self.n_users, 1)
            self._profile_means = self._profiles[:, 0].copy()
            return self
        ids = self._remap(item_features["item_id"], self.item_id_map)
        keep = ids >= 0
        self._feat_ids, self._feat_values = ids[keep], vals[keep]
        first = ~pd.Series(self._feat_ids).duplicated().to_numpy()
        d = len(cols)
        self._F = np.zeros((self.n_items, d))
        self._F[self._feat_ids[first]] = self._feat_values[first]
        self._has = np.zeros(self.n_items, bool)
        self._has[self._feat_ids] = True
        if self.scoring == "neighbors":
            check_similarity_bytes(self.n_items, int(self.max_similarity_bytes), "items")
        eng = self._content_engine()
        P = eng.profiles(self._train_users, self._train_items,
                         self._train_ratings - self.min_rating, self.n_users)
        self._profiles = P.cpu().numpy()
        self._profile_means = (self._profiles.mean(axis=1) if d
                               else np.full(self.n_users, float(self.global_mean)))
        if self.scoring == "neighbors":
            self._neighbour_engine()
        return self

    def predict(self, X: pd.DataFrame, bound_ratings: bool = True) -> list:
        """content_based.py:150-223 for scoring "reference"; the cosine or the
        neighbourhood prediction otherwise (module docstring)."""
        if X.shape[0] == 0:
            return []
        self._fitted()
        X = self._preprocess_data(X=X, type="predict")
        u = X["user_id"].to_numpy(np.int32)
        i = X["item_id"].to_numpy(np.int32)
        if self.scoring == "cosine":
            return self._cosine_engine().predict(u, i, bound_ratings).tolist()
        if self.scoring == "neighbors":
            return self._neighbour_engine().predict(
                i, u, int(self.n_neighbors), self.global_mean, self.min_rating, self.max_rating,
                bound_ratings).tolist()
        if self.scoring != "reference":
            raise ValueError(f"Unknown scoring: {self.scoring!r} (one of {SCORINGS})")
        known = (u >= 0) & (i >= 0)
        pred = np.where(known, self._profile_means[np.where(known, u, 0)],
                        float(self.global_mean))
        if bound_ratings:
            pred = np.clip(pred, self.min_rating, self.max_rating)
        return pred.tolist()

    # ------------------------------------------------------- attributes
    @property
    def item_features(self):
        """The frame given to ``fit`` with ``item_id`` mapped to internal ids
        and the rows of unknown ids dropped (:61-66); feature values as FP64."""
        if self.__dict__.get("_feat_ids") is None:
            return None
        out = pd.DataFrame(self._feat_values, columns=self._feature_cols)
        out.insert(0, "item_id", self._feat_ids.astype(int))
        return out

    @property
    def user_profile_matrix(self):
        """n_users x d FP64 profile rows by internal user id (n_users x 1: the
        mean ratings, when ``fit`` had no item_features); None before fit."""
        return self.__dict__.get("_profiles")

    @property
    def user_profiles(self) -> dict:
        """The reference's dict: internal user id -> FP64 profile row (a
        scalar without item_features); built when read."""
        P = self.__dict__.get("_profiles")
        if P is None:
            return {}
        if self.__dict__.get("_F") is None:
            return {u: P[u, 0] for u in range(len(P))}
        return {u: P[u] for u in range(len(P))}

    @property
    def has_features(self):
        """bool[n_items]: whether the item had a row in item_features."""
        return self.__dict__.get("_has")

    @property
    def item_similarity_matrix(self):
        """n_items x n_items float32 feature cosine in internal-id order,
        fetched from the device (built on the first read unless
        scoring="neighbors" built it in fit); None without item_features."""
        if self.__dict__.get("_F") is None:
            return None
        return self._similarity_device().cpu().numpy()
