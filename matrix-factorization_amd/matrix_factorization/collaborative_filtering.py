"""ItemItemCF and UserUserCF on MI355X: the reference's neighbourhood models
(collaborative_filtering.py:14-368).

One model with the roles swapped.  For ItemItemCF the ENTITIES are the items
and the OTHERS the users; for UserUserCF the other way round.  With n the
number of others, r_ao the rating of entity a by other o (0 where there is
none) and every sum over the stored ratings:

    m_a    = (sum_o r_ao) / n          the pivot's mean, zeros included (:73, :252)
    w_a    = sqrt(max(sum_o r_ao^2 - n m_a^2, 0))
    S[a,b] = (sum_o r_ao r_bo - n m_a m_b) / (w_a w_b),  0 where w_a w_b = 0

which is sklearn's ``cosine_similarity`` of the mean-centred dense matrix
(:87-89, :266-268) without ever forming it; 'cosine' and 'pearson' are the same
computation in the reference (:84-94) and here.  A prediction for target
entity e and other o takes the entities b != e that o rated above 0, keeps the
``n_neighbors`` most similar when there are more, and returns

    m_e + sum S[e,b] (r_bo - m_b) / sum |S[e,b]|

(m_e with no neighbour or a zero denominator, the global mean for an unknown
id).  Statistics, similarity and prediction run on the GPU (mf_cf_stats,
mf_cf_similarity, mf_cf_predict); the similarity is a float32 matrix in HBM,
means and predictions are FP64.  ``recommend_batch``, ``rank_items`` and
``evaluate_topk`` (ranking.RankingMixin, as for the factor models) score every
item for a user in one pass that keeps what the user's pairs share on the chip
(mf_cf_topk, mf_cf_rank): the same predictions bit for bit, ordered by score
descending and internal item id ascending.

``stored_neighbors=M`` (default None: the dense matrix) keeps only each
entity's M best neighbours -- the first min(M, n - 1) entities b != a under
(S[a,b] descending, b ascending), the order of the ``n_neighbors`` cut -- as
n x M ids and float32 similarities (mf_cf_neighbours; 8 M bytes per entity,
the dense row never exists in HBM), so the models fit where the n x n matrix
does not.  A prediction for target e then takes its candidates only from e's
stored row: an entity outside it is no candidate (not "similarity 0");
everything else is unchanged, and with M >= n - 1 every prediction, score,
top-k and rank is the dense model's bit for bit.  ``similarity_neighbors``
returns the stored (ids, sims); the ``*_similarity_matrix`` attributes then
raise rather than densify.

Three deliberate departures from the reference:

1. Ratings stay aligned to their pairs.  The reference's ``fit`` shuffles X in
   ``_preprocess_data`` and then assigns ``y.values`` positionally (:59, :238),
   so it trains on ratings permuted against their pairs.  Here the ratings are
   the ones given for each pair.
2. The target is never its own neighbour.  The reference's "exclude self"
   lines (:167-171, :345-349) index the compressed neighbour list with the
   uncompressed id: on a training pair they drop an unrelated neighbour and
   keep the target at similarity 1.  Pairs whose target the other has not
   rated are unaffected, and parity is claimed on those.
3. Ties at the ``n_neighbors`` cut go to the lower internal id (similarity
   descending, then id ascending); the reference's ``argsort`` (:175, :353)
   leaves their order unspecified.
"""

from __future__ import annotations

import numpy as np
import pandas as pd

from . import _lib
from .neighbours import (DEFAULT_MAX_SIMILARITY_BYTES, MAX_STORED_NEIGHBORS, NeighbourEngine,
                         check_neighbour_bytes, check_similarity_bytes)
from .ranking import RankingMixin
from .recommender_base import RecommenderBase

METRICS = ("cosine", "pearson")


def _warn_if_no_device(name: str) -> None:
    import warnings

    try:
        import torch

        ok = torch.cuda.is_available()
    except Exception:  # pragma: no cover - torch is a dependency
        ok = False
    if not ok:
        warnings.warn(f"{name} loaded, but no HIP device is visible: predict() and recommend() "
                      "will raise MFLibraryError on this host (they run on an AMD Instinct GPU "
                      "through libmf_hip.so); the fitted state is plain NumPy attributes",
                      RuntimeWarning, stacklevel=3)


class _UserQueries:
    """ranking.RankingMixin's backend over a NeighbourEngine: the queries are
    users and the targets all items, whichever of the two the entities are."""

    def __init__(self, engine: NeighbourEngine, side: int, n_neighbors: int, global_mean: float):
        self.engine, self.side = engine, side
        self.n_neighbors, self.global_mean = n_neighbors, global_mean

    def topk(self, uid, amount, ex_ptr=None, ex_items=None):
        return self.engine.topk(uid, self.side, self.n_neighbors, self.global_mean, amount,
                                ex_ptr, ex_items)

    def rank(self, uid, tgt_ptr, tgt_items, ex_ptr=None, ex_items=None):
        return self.engine.rank(uid, self.side, self.n_neighbors, self.global_mean, tgt_ptr,
                                tgt_items, ex_ptr, ex_items)


class _NeighbourhoodCF(RankingMixin, RecommenderBase):
    """Shared body of ItemItemCF / UserUserCF; ``_ENTITY`` names the side the
    similarity is taken over."""

    _ENTITY = "item"

    def __init__(self, min_rating: float = 0, max_rating: float = 5, n_neighbors: int = 50,
                 similarity_metric: str = "cosine", verbose: int = 0, device=None,
                 max_similarity_bytes: int = DEFAULT_MAX_SIMILARITY_BYTES,
                 stored_neighbors=None):
        super().__init__(min_rating=min_rating, max_rating=max_rating, verbose=verbose)
        self.n_neighbors = n_neighbors
        self.similarity_metric = similarity_metric
        self.device = device
        self.max_similarity_bytes = max_similarity_bytes
        self.stored_neighbors = stored_neighbors

    # stored_neighbors=None is the dense model unchanged in every respect, its
    # parameter dict included: the parameter is listed once it is set
    def get_params(self, deep: bool = True) -> dict:
        params = super().get_params(deep=deep)
        if params.get("stored_neighbors") is None:
            params.pop("stored_neighbors", None)
        return params

    def set_params(self, **params):
        if "stored_neighbors" in params:
            self.stored_neighbors = params.pop("stored_neighbors")
        return super().set_params(**params)

    # ------------------------------------------------------------ state
    def _sides(self):
        """(entity ids, other ids, n_entities, n_others) of the fitted triples."""
        if self._ENTITY == "item":
            return self._train_items, self._train_users, self.n_items, self.n_users
        return self._train_users, self._train_items, self.n_users, self.n_items

    def _fitted_engine(self) -> NeighbourEngine:
        """The device state, rebuilt from the triples when there is none (first
        use after unpickling)."""
        eng = self.__dict__.get("_engine")
        if eng is None:
            if self.__dict__.get("_train_users") is None:
                raise AttributeError(f"{type(self).__name__} is not fitted")
            ent, oth, n_ent, n_oth = self._sides()
            eng = NeighbourEngine(ent, oth, self._train_ratings, n_ent, n_oth, self.device,
                                  int(self.max_similarity_bytes), what=self._ENTITY + "s",
                                  stored_neighbors=self.stored_neighbors)
            self._engine = eng
        return eng

    def __getstate__(self):
        # NumPy and builtins only: id maps, triples, means, global mean; the
        # similarity is recomputed on the first predict after loading
        state = self.__dict__.copy()
        state.pop("_engine", None)
        state.pop("_maps_pending", None)
        state.pop("_defer_maps", None)
        return state

    def __setstate__(self, state):
        for key, default in (("device", None),
                             ("max_similarity_bytes", DEFAULT_MAX_SIMILARITY_BYTES),
                             ("stored_neighbors", None)):
            state.setdefault(key, default)
        self.__dict__.update(state)
        _warn_if_no_device(type(self).__name__)

    def _ranking_backend(self) -> _UserQueries:
        """recommend_batch / rank_items / evaluate_topk (ranking.RankingMixin):
        a user is an OTHER of the item-item model and an ENTITY of the
        user-user one; the engine is rebuilt after unpickling, as for predict."""
        side = _lib.MF_CF_QUERY_OTHER if self._ENTITY == "item" else _lib.MF_CF_QUERY_ENTITY
        return _UserQueries(self._fitted_engine(), side, int(self.n_neighbors),
                            float(self.global_mean))

    # -------------------------------------------------------------- API
    def fit(self, X: pd.DataFrame, y: pd.Series):
        """collaborative_filtering.py:49-78 / :228-257: ``_preprocess_data``
        (the reference's one RNG draw, id maps and duplicate check), the
        global mean, then means and similarity on the GPU."""
        if (isinstance(self.n_neighbors, bool) or not isinstance(self.n_neighbors, (int, np.integer))
                or self.n_neighbors < 1):
            raise ValueError(f"n_neighbors must be an integer >= 1, got {self.n_neighbors!r}")
        M = self.stored_neighbors
        if M is not None and (isinstance(M, bool) or not isinstance(M, (int, np.integer))
                              or not 1 <= M <= MAX_STORED_NEIGHBORS):
            raise ValueError(f"stored_neighbors must be None or an integer in "
                             f"[1, {MAX_STORED_NEIGHBORS}], got {M!r}")
        X = self._preprocess_data(X=X, y=y, type="fit")
        self.global_mean = X["rating"].mean()
        if self.similarity_metric not in METRICS:
            raise ValueError(f"Unknown similarity metric: {self.similarity_metric}")
        self._engine = None
        self._train_users = X["user_id"].to_numpy(np.int32)
        self._train_items = X["item_id"].to_numpy(np.int32)
        self._train_ratings = X["rating"].to_numpy(np.float64)
        n_ent = self._sides()[2]
        if M is None:
            check_similarity_bytes(n_ent, int(self.max_similarity_bytes), self._ENTITY + "s")
        else:
            check_neighbour_bytes(n_ent, int(M), int(self.max_similarity_bytes),
                                  self._ENTITY + "s")
        eng = self._fitted_engine()
        self._means = eng.mean.cpu().numpy()
        return self

    def predict(self, X: pd.DataFrame, bound_ratings: bool = True) -> list:
        """collaborative_filtering.py:98-131 / :276-309."""
        if X.shape[0] == 0:
            return []
        X = self._preprocess_data(X=X, type="predict")
        u = X["user_id"].to_numpy(np.int32)
        i = X["item_id"].to_numpy(np.int32)
        ent, oth = (i, u) if self._ENTITY == "item" else (u, i)
        pred = self._fitted_engine().predict(ent, oth, int(self.n_neighbors), self.global_mean,
                                             self.min_rating, self.max_rating, bound_ratings)
        return pred.tolist()

    # ------------------------------------------------------- attributes
    def _mean_ratings(self):
        m = self.__dict__.get("_means")
        if m is None:
            return None
        return pd.Series(m, index=pd.RangeIndex(len(m), name=self._ENTITY + "_id"))

    def _similarity_matrix(self):
        if self.__dict__.get("_train_users") is None:
            return None
        if self.stored_neighbors is not None:
            raise AttributeError(
                f"{type(self).__name__}(stored_neighbors={self.stored_neighbors!r}) keeps no "
                f"dense {self._ENTITY}_similarity_matrix; use similarity_neighbors")
        eng = self._fitted_engine()
        return eng.S.cpu().numpy()

    @property
    def similarity_neighbors(self):
        """(ids int32, sims float32), each n_entities x stored_neighbors, as
        stored: internal ids, every row id-ascending, padded with -1 / 0; None
        before ``fit``.  A dense model (stored_neighbors=None) has none."""
        if self.stored_neighbors is None:
            raise AttributeError(
                f"{type(self).__name__} with stored_neighbors=None keeps the dense matrix; use "
                f"{self._ENTITY}_similarity_matrix")
        if self.__dict__.get("_train_users") is None:
            return None
        eng = self._fitted_engine()
        return eng.nbr_ids.cpu().numpy(), eng.nbr_sims.cpu().numpy()

    @property
    def user_item_matrix(self):
        """The dense users x items frame of the reference's pivot (:62-67),
        0 where there is no rating; built on the host when read."""
        if self.__dict__.get("_train_users") is None:
            return None
        R = np.zeros((self.n_users, self.n_items))
        R[self._train_users, self._train_items] = self._train_ratings
        return pd.DataFrame(R, index=pd.RangeIndex(self.n_users, name="user_id"),
                            columns=pd.RangeIndex(self.n_items, name="item_id"))


class ItemItemCF(_NeighbourhoodCF):
    """Item-item collaborative filtering (collaborative_filtering.py:193-368):
    a user's rating of an item is predicted from that user's ratings of the
    ``n_neighbors`` most similar items.

    Arguments (reference defaults): min_rating=0, max_rating=5,
    n_neighbors=50, similarity_metric='cosine' | 'pearson' (the same
    computation, as in the reference), verbose=0; plus device and
    max_similarity_bytes (default 16 GiB: ``fit`` refuses, with a ValueError
    naming the size and before allocating anything, an n_items x n_items
    float32 similarity larger than this) and stored_neighbors (default None:
    the dense matrix; an integer M in [1, 4096] keeps each item's M best
    neighbours instead -- module docstring -- and the budget then covers the
    8 M n_items bytes of the lists plus the workspace that builds them).

    Attributes after fit: item_mean_ratings (float64 Series by internal item
    id), item_similarity_matrix (float32 ndarray fetched from the device on
    access; AttributeError with stored_neighbors), similarity_neighbors (the
    stored (ids, sims); AttributeError without), user_item_matrix (dense frame,
    built on the host when read).

    Departures from the reference (module docstring): ratings stay aligned to
    their pairs; the target item is never its own neighbour; ties at the
    n_neighbors cut go to the lower internal id.
    """

    _ENTITY = "item"

    def __init__(self, min_rating: float = 0, max_rating: float = 5, n_neighbors: int = 50,
                 similarity_metric: str = "cosine", verbose: int = 0, device=None,
                 max_similarity_bytes: int = DEFAULT_MAX_SIMILARITY_BYTES,
                 stored_neighbors=None):
        super().__init__(min_rating=min_rating, max_rating=max_rating, n_neighbors=n_neighbors,
                         similarity_metric=similarity_metric, verbose=verbose, device=device,
                         max_similarity_bytes=max_similarity_bytes,
                         stored_neighbors=stored_neighbors)

    @property
    def item_mean_ratings(self):
        return self._mean_ratings()

    @property
    def item_similarity_matrix(self):
        return self._similarity_matrix()


class UserUserCF(_NeighbourhoodCF):
    """User-user collaborative filtering (collaborative_filtering.py:14-190):
    a user's rating of an item is predicted from the ratings the
    ``n_neighbors`` most similar users gave that item.

    Arguments (reference defaults): min_rating=0, max_rating=5,
    n_neighbors=50, similarity_metric='cosine' | 'pearson' (the same
    computation, as in the reference), verbose=0; plus device and
    max_similarity_bytes (default 16 GiB: ``fit`` refuses, with a ValueError
    naming the size and before allocating anything, an n_users x n_users
    float32 similarity larger than this) and stored_neighbors (default None:
    the dense matrix; an integer M in [1, 4096] keeps each user's M best
    neighbours instead -- module docstring -- and the budget then covers the
    8 M n_users bytes of the lists plus the workspace that builds them).

    Attributes after fit: user_mean_ratings (float64 Series by internal user
    id), user_similarity_matrix (float32 ndarray fetched from the device on
    access; AttributeError with stored_neighbors), similarity_neighbors (the
    stored (ids, sims); AttributeError without), user_item_matrix (dense frame,
    built on the host when read).

    Departures from the reference (module docstring): ratings stay aligned to
    their pairs; the target user is never their own neighbour; ties at the
    n_neighbors cut go to the lower internal id.
    """

    _ENTITY = "user"

    def __init__(self, min_rating: float = 0, max_rating: float = 5, n_neighbors: int = 50,
                 similarity_metric: str = "cosine", verbose: int = 0, device=None,
                 max_similarity_bytes: int = DEFAULT_MAX_SIMILARITY_BYTES,
                 stored_neighbors=None):
        super().__init__(min_rating=min_rating, max_rating=max_rating, n_neighbors=n_neighbors,
                         similarity_metric=similarity_metric, verbose=verbose, device=device,
                         max_similarity_bytes=max_similarity_bytes,
                         stored_neighbors=stored_neighbors)

    @property
    def user_mean_ratings(self):
        return self._mean_ratings()

    @property
    def user_similarity_matrix(self):
        return self._similarity_matrix()
