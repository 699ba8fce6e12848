"""HybridRecommender on MI355X: embedding retrieval, then a factor-model
rerank -- the path the reference's consumer ships
(project_template/pipeline/evaluate_hybrid.py:107-159, app/retrieval.py).

Per user, with E the float32 item-embedding rows ("the index"):

1. profile: the mean of the index rows of the user's history items that are in
   the index, normalised to unit length (evaluate_hybrid.py:122-130);
2. retrieval: the ``candidate_k`` index rows with the largest dot product with
   the profile -- the cosine when the rows have unit length (:133-136);
3. the rows of the user's history items are dropped (:137-138) -- after the
   retrieval, so fewer than ``candidate_k`` candidates can remain;
4. the survivors are scored by ``model.predict(..., bound_ratings=False)``,
   cast to float32 (:147-149); without a model every score is 0;
5. they are ranked by ``alpha * minmax(model) + (1 - alpha) * minmax(cosine)``
   in float32 (:72-79, :151-152).

Steps 1 and 2 run through the kernels ContentBasedRecommender's cosine scoring
uses (mf_content_profiles, mf_content_normalize, mf_topk on a DeviceModel
whose rows are the profiles and the index); steps 3 to 5 are one pass of
mf_hybrid_rerank, a workgroup per user.  Candidates and similarities stay on
the device between the two stages; the model's parameters are read through its
own predictor (``_model_args``) and are not copied.

Three deliberate departures from the reference:

1. Equal blended scores rank in retrieval order (the stable order); the
   reference's ``np.argsort(-score)`` leaves their order unspecified.
2. The profile mean is taken in FP64 and rounded once to float32 after the
   normalisation; the reference averages in float32.  The two differ by
   rounding only.
3. ``fit`` takes the histories once, and duplicate (user, item) rows in them
   count once; the reference re-splits the ratings per evaluation call.
"""

from __future__ import annotations

from typing import Union

import numpy as np
import pandas as pd
import torch

from . import _lib
from .collaborative_filtering import _warn_if_no_device
from .content_based import ContentBasedRecommender, ContentEngine
from .device_model import DeviceModel, _VOID, _tp, resolve_device
from .utils import ranking_metrics_from_ranks

MAX_CANDIDATES = 2048                  # mf_topk's largest amount
_NOT_RECOMMENDED = np.iinfo(np.int32).max


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _plain_ids(values) -> np.ndarray:
    """External ids as a typed NumPy array (integers, or '<U' strings where
    pandas held them as objects), so that pickles carry no object arrays."""
    a = np.asarray(values)
    if a.dtype == object:
        b = np.asarray(a.tolist())
        if b.dtype != object and b.shape == a.shape and set(map(type, a.tolist())) <= {str}:
            a = b
    return a


class HybridRecommender:
    """Embedding retrieval + model rerank (module docstring).

    Arguments: model (a fitted KernelMF, ALSMF, ImplicitALSMF or BPRMF, or
    None: pure embedding retrieval, the reference's ``model is None`` branch),
    alpha (weight of the model term, in [0, 1], default 0.7), candidate_k
    (1 .. 2048, default 200), min_profile_items (>= 1: a user with fewer
    history items in the index has no profile, gets no recommendations and is
    left out of the evaluation), normalize_items (True: the embedding rows are
    normalised to unit length by mf_content_normalize; False: they are used as
    given, cast to float32 -- the reference assumes a pre-normalised index),
    device (the model's, when a model is given).

    Attributes after fit: index_item_ids (the index's item ids, row order),
    item_embeddings (float32 index rows), user_ids, user_profiles (float32,
    unit length, a zero row for a user without a profile), has_profile.
    """

    def __init__(self, model=None, alpha: float = 0.7, candidate_k: int = 200,
                 min_profile_items: int = 1, normalize_items: bool = True, device=None):
        self.model = model
        self.alpha = alpha
        self.candidate_k = candidate_k
        self.min_profile_items = min_profile_items
        self.normalize_items = normalize_items
        self.device = device
        self._check_arguments(fitted_model=False)

    # users per mf_hybrid_rerank launch (the output does not depend on it)
    rerank_chunk = 1 << 16

    def _check_arguments(self, fitted_model: bool) -> None:
        ck = self.candidate_k
        if not _is_int(ck) or not 1 <= ck <= MAX_CANDIDATES:
            raise ValueError(f"candidate_k must be an integer in [1, {MAX_CANDIDATES}], got {ck!r}")
        a = self.alpha
        if (isinstance(a, bool) or not isinstance(a, (int, float, np.integer, np.floating))
                or not 0.0 <= float(a) <= 1.0):
            raise ValueError(f"alpha must be a number in [0, 1], got {a!r}")
        mp = self.min_profile_items
        if not _is_int(mp) or mp < 1:
            raise ValueError(f"min_profile_items must be an integer >= 1, got {mp!r}")
        m = self.model
        if m is not None:
            if not callable(getattr(m, "_predictor", None)):
                raise ValueError("model must be a KernelMF-family estimator (KernelMF, ALSMF, "
                                 f"ImplicitALSMF, BPRMF) or None, got {type(m).__name__}")
            if fitted_model and (getattr(m, "user_features", None) is None
                                 or getattr(m, "item_id_map", None) is None):
                raise ValueError("model is not fitted: fit it before HybridRecommender.fit")

    # ------------------------------------------------------------ state
    _DEVICE_STATE = ("_engine", "_row_item", "_row_item_key", "_user_index", "_item_index")

    def __getstate__(self):
        # NumPy and builtins only (and the model's own such state); the
        # engines are rebuilt on first use
        state = self.__dict__.copy()
        for key in self._DEVICE_STATE:
            state.pop(key, None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        _warn_if_no_device(type(self).__name__)

    def _fitted(self) -> None:
        if self.__dict__.get("_profiles") is None:
            raise AttributeError(f"{type(self).__name__} is not fitted")

    @property
    def index_item_ids(self):
        return self.__dict__.get("_index_ids")

    @property
    def item_embeddings(self):
        return self.__dict__.get("_E")

    @property
    def user_ids(self):
        return self.__dict__.get("_user_ids")

    @property
    def user_profiles(self):
        return self.__dict__.get("_profiles")

    @property
    def has_profile(self):
        return self.__dict__.get("_has_profile")

    def _lookup(self, name: str, ids, labels) -> np.ndarray:
        idx = self.__dict__.get(name)
        if idx is None:
            idx = self.__dict__[name] = pd.Index(ids)
        return idx.get_indexer(pd.Index(_plain_ids(labels)))

    def _user_codes(self, labels) -> np.ndarray:
        """Position of each label in ``user_ids``, -1 where unknown."""
        return self._lookup("_user_index", self._user_ids, labels)

    def _index_rows(self, item_ids) -> np.ndarray:
        """Index row of each item id, -1 where the item is not in the index."""
        return self._lookup("_item_index", self._index_ids, item_ids)

    # -------------------------------------------------------------- fit
    def fit(self, X: pd.DataFrame, item_embeddings: pd.DataFrame):
        """X: DataFrame[user_id, item_id], the users' histories (the
        reference's ``train_items``); item_embeddings: ``item_id`` plus numeric
        columns, as ContentBasedRecommender takes ``item_features``."""
        self._check_arguments(fitted_model=True)
        for col in ("user_id", "item_id"):
            if col not in X.columns:
                raise ValueError(f"X must contain '{col}' column")
        _, vals = ContentBasedRecommender._feature_values(item_embeddings)
        d = vals.shape[1]
        kmax = _lib.load().mf_max_factors()
        if not 1 <= d <= kmax:
            raise ValueError(f"item_embeddings has d = {d} numeric columns; 1 .. "
                             f"mf_max_factors() = {kmax} are supported")
        ids = _plain_ids(item_embeddings["item_id"].to_numpy())
        first = ~pd.Series(ids).duplicated().to_numpy()
        if not first.any():
            raise ValueError("item_embeddings holds no rows")
        for key in self._DEVICE_STATE + ("_profiles",):
            self.__dict__.pop(key, None)
        self._index_ids = ids[first]
        vals = vals[first]
        n_rows = len(self._index_ids)
        dev = resolve_device(self.device)
        if self.normalize_items:
            E = ContentEngine(vals, np.ones(n_rows, bool), dev)
            self._E = E.normalize(E.F).cpu().numpy()
        else:
            self._E = np.ascontiguousarray(vals, np.float32)
        # histories: distinct (user, index row) pairs, rows sorted per user
        ucode, ulabel = pd.factorize(_plain_ids(X["user_id"].to_numpy()))
        self._user_ids = _plain_ids(ulabel)
        n_users = len(self._user_ids)
        rows = self._index_rows(X["item_id"].to_numpy())
        keep = rows >= 0
        pair = np.unique(ucode[keep].astype(np.int64) * n_rows + rows[keep])
        hu, hr = pair // n_rows, (pair % n_rows).astype(np.int32)
        self._hist_ptr = np.zeros(n_users + 1, np.int64)
        np.cumsum(np.bincount(hu, minlength=n_users), out=self._hist_ptr[1:])
        self._hist_rows = hr
        self._has_profile = np.diff(self._hist_ptr) >= int(self.min_profile_items)
        # profiles: FP64 mean of the float32 index rows, normalised to float32
        ce = ContentEngine(self._E.astype(np.float64), np.ones(n_rows, bool), dev)
        live = self._has_profile[hu]
        P = ce.profiles(hu[live], hr[live], np.ones(int(live.sum())), n_users)
        self._profiles = ce.normalize(P).cpu().numpy()
        return self

    # ---------------------------------------------------------- engines
    def _retrieval_engine(self) -> DeviceModel:
        """A factor model whose rows are the profiles and the index rows: its
        mf_topk is the retrieval."""
        eng = self.__dict__.get("_engine")
        if eng is None:
            n_users, d = self._profiles.shape
            n_rows = len(self._E)
            dpad = (d + 3) // 4 * 4
            pad = lambda a: np.ascontiguousarray(  # noqa: E731
                np.pad(a, ((0, 0), (0, dpad - d))), np.float32)
            eng = DeviceModel(n_users, n_rows, dpad, "linear", "float32", self.device,
                              min_rating=0.0, max_rating=1.0, global_mean=0.0)
            eng.load_params(pad(self._profiles), pad(self._E), np.zeros(n_users),
                            np.zeros(n_rows))
            self._engine = eng
        return eng

    def _model_side(self, eng: DeviceModel, labels: np.ndarray):
        """(model engine, device int32 model user ids of ``labels``, device
        int32 model item id per index row); (None, None, None) without a model."""
        m = self.model
        if m is None:
            return None, None, None
        if getattr(m, "user_features", None) is None:
            raise ValueError("model is not fitted")
        me = m._predictor()
        if me.dev != eng.dev:
            raise ValueError(f"model lives on {me.dev}, the index on {eng.dev}: give both the "
                             "same device")
        uid = m._remap(pd.Series(labels, dtype=object), m.user_id_map).astype(np.int32)
        key = id(m.item_id_map), len(m.item_id_map)
        if self.__dict__.get("_row_item") is None or self.__dict__.get("_row_item_key") != key:
            ri = m._remap(pd.Series(self._index_ids, dtype=object), m.item_id_map)
            self._row_item = torch.from_numpy(ri.astype(np.int32)).to(eng.dev)
            self._row_item_key = key
        return me, torch.from_numpy(uid).to(eng.dev), self._row_item

    # ------------------------------------------------------- the passes
    def _rerank(self, ucodes: np.ndarray, amount):
        """Both stages for the users ``ucodes`` (positions in ``user_ids``, all
        with a profile).  ``amount`` None: the whole candidate list.  Host
        arrays (rows [n, amount], scores, model scores, similarities, kept
        counts [n])."""
        self._fitted()
        eng = self._retrieval_engine()
        nq = len(ucodes)
        n_cand = min(int(self.candidate_k), eng.n_items)
        amount = n_cand if amount is None else max(0, min(int(amount), n_cand))
        if nq == 0:
            z = np.zeros((0, amount), np.float32)
            return np.zeros((0, amount), np.int32), z, z, z, np.zeros(0, np.int32)
        ucodes = np.ascontiguousarray(ucodes, np.int64)
        q = eng.topk_prepare(ucodes.astype(np.int32), n_cand)
        eng.topk_launch(q)
        eng.topk_finish(q)
        dev = eng.dev
        cnt = np.diff(self._hist_ptr)[ucodes]
        ex_ptr = np.zeros(nq + 1, np.int64)
        np.cumsum(cnt, out=ex_ptr[1:])
        src = np.repeat(self._hist_ptr[ucodes] - ex_ptr[:-1], cnt) + np.arange(ex_ptr[-1])
        ex_rows = self._hist_rows[src] if len(src) else np.zeros(1, np.int32)
        d_ptr = torch.from_numpy(ex_ptr).to(dev)
        d_ex = torch.from_numpy(np.ascontiguousarray(ex_rows, np.int32)).to(dev)
        me, d_uid, d_row_item = self._model_side(eng, self._user_ids[ucodes])
        new = lambda dt: torch.empty((nq, amount), dtype=dt, device=dev)  # noqa: E731
        o_rows, o_sc, o_mo, o_si = (new(torch.int32), new(torch.float32), new(torch.float32),
                                    new(torch.float32))
        o_m = torch.empty(nq, dtype=torch.int32, device=dev)
        off = lambda t, n: _VOID(t.data_ptr() + t.element_size() * n)  # noqa: E731
        chunk = max(1, int(self.rerank_chunk))
        with torch.cuda.device(dev):
            for q0 in range(0, nq, chunk):
                q1 = min(nq, q0 + chunk)
                model = ((None, 0.0, None, None, None, None, 0, 0, _lib.MF_LINEAR, _lib.MF_F32,
                          0.0, 0.0, 0.0) if me is None else
                         (off(d_uid, q0), *me._model_args()))
                # exclusion offsets stay absolute: the chunk's ptr array starts at row q0
                _lib.call("mf_hybrid_rerank", model[0], q1 - q0, off(q["items"], n_cand * q0),
                          off(q["scores"], n_cand * q0), n_cand,
                          None if d_row_item is None else _tp(d_row_item), eng.n_items,
                          *model[1:], off(d_ptr, q0), _tp(d_ex), float(self.alpha), amount, None,
                          off(o_rows, amount * q0), off(o_sc, amount * q0),
                          off(o_mo, amount * q0), off(o_si, amount * q0), off(o_m, q0),
                          eng.stream)
        return (o_rows.cpu().numpy(), o_sc.cpu().numpy(), o_mo.cpu().numpy(),
                o_si.cpu().numpy(), o_m.cpu().numpy())

    def _queries(self, labels):
        """Positions in ``labels`` of the users with a profile, and their
        positions in ``user_ids``."""
        self._fitted()
        codes = self._user_codes(labels)
        ok = codes >= 0
        ok[ok] = self._has_profile[codes[ok]]
        pos = np.flatnonzero(ok)
        return pos, codes[pos]

    # -------------------------------------------------------------- API
    def recommend_batch(self, users, amount: int = 10) -> pd.DataFrame:
        """The best ``amount`` reranked candidates of each user:
        DataFrame[user_id, item_id, score, model_score, similarity] ordered by
        user, then rank; ``score`` is the blend, the other two its raw terms.
        A user that ``fit`` did not see or that has no profile gets no rows; a
        user gets fewer than ``amount`` rows when fewer candidates remain."""
        users = list(users)
        pos, codes = self._queries(users)
        rows, score, model, sims, _ = self._rerank(codes, amount)
        valid = rows >= 0
        return pd.DataFrame({
            "user_id": np.repeat(_plain_ids(users)[pos], valid.sum(axis=1)),
            "item_id": self._index_ids[rows[valid]],
            "score": score[valid],
            "model_score": model[valid],
            "similarity": sims[valid],
        })

    def recommend(self, user, amount: int = 10) -> pd.DataFrame:
        """``recommend_batch`` for one user."""
        return self.recommend_batch([user], amount)

    def _positions(self, X: pd.DataFrame):
        """Per row of X the code of its user among X's distinct users and the
        0-based position of its item in the user's reranked list (-1: not in
        it); per distinct user the kept-candidate count (0: no profile)."""
        ucode, ulabel = pd.factorize(_plain_ids(X["user_id"].to_numpy()))
        pos, codes = self._queries(ulabel)
        rows, _, _, _, m = self._rerank(codes, None)
        n_rows = len(self._index_ids)
        cand = np.zeros(len(ulabel), np.int32)
        cand[pos] = m
        rank = np.full(len(ucode), -1, np.int32)
        qi, ci = np.nonzero(rows >= 0)
        if len(ucode) and len(qi):
            # (user, row) -> list position, looked up in the sorted pairs
            have = pos[qi].astype(np.int64) * n_rows + rows[qi, ci]
            order = np.argsort(have, kind="stable")
            have, ci = have[order], ci[order]
            trow = self._index_rows(X["item_id"].to_numpy())
            want = ucode.astype(np.int64) * n_rows + np.maximum(trow, 0)
            at = np.minimum(np.searchsorted(have, want), len(have) - 1)
            hit = (trow >= 0) & (have[at] == want)
            rank[hit] = ci[at[hit]]
        return ucode, rank, ulabel, cand

    def rank_items(self, X: pd.DataFrame) -> pd.DataFrame:
        """Position of each (user_id, item_id) row of X in the user's whole
        reranked candidate list (0 = first).  An item that was not retrieved,
        was dropped or is not in the index is not recommended: rank -1.
        Returns DataFrame[user_id, item_id, rank, n_candidates] in X's row
        order; n_candidates is the number of candidates kept (0 for a user
        without a profile)."""
        ucode, rank, _, cand = self._positions(X)
        return pd.DataFrame({
            "user_id": X["user_id"].to_numpy(),
            "item_id": X["item_id"].to_numpy(),
            "rank": rank,
            "n_candidates": cand[ucode] if len(ucode) else np.zeros(0, np.int32),
        })

    def evaluate_topk(self, X: pd.DataFrame, k: Union[int, list] = 10):
        """Precision, recall, NDCG, MAP and MRR at ``k`` of the held-out pairs
        X (DataFrame[user_id, item_id]) against each user's reranked list, by
        ``utils.ranking_metrics_from_ranks``: evaluate_hybrid.py:152-167.  A
        held-out item that is not in the list counts as a miss, and
        n_relevant is the user's number of held-out rows; users without a
        profile or without a kept candidate are left out (:118-141).  AUC is
        not reported: it has no meaning under a candidate cut.  ``k`` may be
        a list: one GPU pass, a dict of results keyed by k."""
        X = X[["user_id", "item_id"]].drop_duplicates()
        ucode, rank, ulabel, cand = self._positions(X)
        use = cand[ucode] > 0 if len(ucode) else np.zeros(0, bool)
        ucode, rank = ucode[use], rank[use]
        order = np.argsort(ucode, kind="stable")
        cnt = np.bincount(ucode, minlength=len(ulabel))
        sel = cnt > 0
        ptr = np.zeros(int(sel.sum()) + 1, np.int64)
        np.cumsum(cnt[sel], out=ptr[1:])
        r = np.where(rank[order] >= 0, rank[order], _NOT_RECOMMENDED)

        def one(kk: int) -> dict:
            out = ranking_metrics_from_ranks(r, ptr, cand[sel], cnt[sel], kk)
            out.pop("auc", None)
            return out

        if isinstance(k, (int, np.integer)):
            return one(int(k))
        return {int(kk): one(int(kk)) for kk in k}
