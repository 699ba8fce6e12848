"""Device-side state of the neighbourhood models (ItemItemCF / UserUserCF).

One engine serves both classes: the ENTITIES are the items (ItemItemCF) or the
users (UserUserCF), the OTHERS are the other side.  The fitted triples are
sorted into both CSR orientations on the device (entity-major with each list
ascending in the other's id, other-major with each list ascending in the
entity's id: the order mf_cf_similarity's bitwise symmetry rests on), the
statistics and the similarity are computed once (mf_cf_stats,
mf_cf_similarity), and predict() scores pairs in chunks (mf_cf_predict).
scores() / topk() / rank() take every target for a batch of queries in one
pass (mf_cf_scores, mf_cf_topk, mf_cf_rank): the same predictions bit for bit,
the queries in chunks that keep the key workspace within ``topk_ws_budget``.
Ratings are float32 on the device; means, norms and predictions are FP64.

``stored_neighbors=M`` keeps, in place of the dense n_entities x n_entities
matrix, each entity's M best neighbours (mf_cf_neighbours: ids and float32
similarities, id-ascending rows, 8 M bytes per entity; the dense row never
exists in HBM) and routes predict / scores / topk / rank to the list variants
(mf_cf_*_nbr): a candidate b counts for target e only when b is in e's stored
row.  With M >= n_entities - 1 every result is the dense model's, bit for bit.
"""

from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .device_model import _VOID, _tp, exclusion_csr, resolve_device, target_csr

DEFAULT_MAX_SIMILARITY_BYTES = 16 << 30      # policy, not a measurement
PREDICT_CHUNK = 1 << 20                      # pairs per mf_cf_predict launch (<= 2^25)


def similarity_bytes(n_entities: int) -> int:
    return 4 * int(n_entities) * int(n_entities)


def check_similarity_bytes(n_entities: int, max_bytes: int, what: str = "entities") -> None:
    """Refuse, before anything is allocated, a similarity matrix larger than
    ``max_bytes``."""
    need = similarity_bytes(n_entities)
    if need > max_bytes:
        raise ValueError(
            f"the {n_entities} x {n_entities} float32 similarity matrix of {n_entities} {what} "
            f"needs {need} bytes ({need / 2**30:.2f} GiB), more than max_similarity_bytes="
            f"{max_bytes}")


MAX_STORED_NEIGHBORS = 4096                  # a stored row is at most 32 KiB (mf_cf_neighbours)


def neighbour_bytes(n_entities: int, stored_neighbors: int) -> tuple:
    """(bytes of the stored lists, bytes of mf_cf_neighbours' workspace)."""
    ws = int(_lib.load().mf_cf_neighbours_workspace_bytes(int(n_entities), int(stored_neighbors)))
    return 8 * int(n_entities) * int(stored_neighbors), ws


def check_neighbour_bytes(n_entities: int, stored_neighbors: int, max_bytes: int,
                          what: str = "entities") -> None:
    """Refuse, before anything is allocated, stored neighbour lists that, with
    the workspace that builds them, are larger than ``max_bytes``."""
    lists, ws = neighbour_bytes(n_entities, stored_neighbors)
    if lists + ws > max_bytes:
        raise ValueError(
            f"the {stored_neighbors} stored neighbours of each of {n_entities} {what} need "
            f"{lists} bytes and {ws} bytes of workspace to build, {lists + ws} bytes "
            f"({(lists + ws) / 2**30:.2f} GiB), more than max_similarity_bytes={max_bytes}")


class NeighbourEngine:
    """CSR lists, statistics and similarity of one fitted neighbourhood model.

    ent, oth, r: the training triples (internal ids, one rating per pair).
    Attributes: mean, norm (float64 device tensors, n_entities), S (float32
    device tensor, n_entities x n_entities).  With ``stored_neighbors=M`` S is
    None and nbr_ids (int32) / nbr_sims (float32), n_entities x M device
    tensors, hold each entity's M best neighbours by id ascending (-1 / 0
    padding).  ``similarity=`` (a float32 device tensor, n_entities x
    n_entities) is taken as S in place of mf_cf_similarity's."""

    def __init__(self, ent: np.ndarray, oth: np.ndarray, r: np.ndarray, n_entities: int,
                 n_others: int, device=None,
                 max_similarity_bytes: int = DEFAULT_MAX_SIMILARITY_BYTES,
                 pass_cols: int = 0, what: str = "entities", stored_neighbors=None,
                 similarity=None):
        self.stored = None if stored_neighbors is None else int(stored_neighbors)
        if similarity is not None:
            if self.stored is not None:
                raise ValueError("a precomputed similarity is dense: stored_neighbors must be None")
            if (not isinstance(similarity, torch.Tensor) or similarity.dtype != torch.float32
                    or tuple(similarity.shape) != (int(n_entities), int(n_entities))):
                raise ValueError(f"similarity must be a float32 tensor of shape "
                                 f"({n_entities}, {n_entities})")
        if self.stored is None:
            check_similarity_bytes(n_entities, max_similarity_bytes, what)
        else:
            if not 1 <= self.stored <= MAX_STORED_NEIGHBORS:
                raise ValueError(f"stored_neighbors must be in [1, {MAX_STORED_NEIGHBORS}] or "
                                 f"None, got {stored_neighbors!r}")
            check_neighbour_bytes(n_entities, self.stored, max_similarity_bytes, what)
        ent = np.asarray(ent, dtype=np.int64)
        oth = np.asarray(oth, dtype=np.int64)
        if len(ent) and (ent.min() < 0 or ent.max() >= n_entities
                         or oth.min() < 0 or oth.max() >= n_others):
            raise ValueError("rating ids outside [0, n_entities) x [0, n_others)")
        self.dev = resolve_device(device)
        self.n_entities, self.n_others = int(n_entities), int(n_others)
        with torch.cuda.device(self.dev):
            d_ent = torch.from_numpy(ent).to(self.dev)
            d_oth = torch.from_numpy(oth).to(self.dev)
            d_r = torch.from_numpy(np.asarray(r, dtype=np.float32)).to(self.dev)
            self.entity_csr = self._csr(d_ent, d_oth, d_r, self.n_entities, self.n_others)
            self.other_csr = self._csr(d_oth, d_ent, d_r, self.n_others, self.n_entities)
            self.mean = torch.empty(self.n_entities, dtype=torch.float64, device=self.dev)
            self.norm = torch.empty(self.n_entities, dtype=torch.float64, device=self.dev)
            eptr, eoth, er = self.entity_csr
            optr, oent, orr = self.other_csr
            _lib.call("mf_cf_stats", _tp(eptr), _tp(er), self.n_entities, self.n_others,
                      _lib.MF_F32, _tp(self.mean), _tp(self.norm), self.stream)
            lists = (_tp(eptr), _tp(eoth), _tp(er), _tp(optr), _tp(oent), _tp(orr),
                     self.n_entities, self.n_others, _lib.MF_F32, _tp(self.mean), _tp(self.norm),
                     int(pass_cols))
            self.S = self.nbr_ids = self.nbr_sims = None
            if similarity is not None:
                # the caller's matrix in place of the rating similarity
                self.S = similarity.to(self.dev).contiguous()
            elif self.stored is None:
                self.S = torch.empty((self.n_entities, self.n_entities), dtype=torch.float32,
                                     device=self.dev)
                _lib.call("mf_cf_similarity", *lists, _tp(self.S), self.stream)
            else:
                shape = (self.n_entities, self.stored)
                self.nbr_ids = torch.empty(shape, dtype=torch.int32, device=self.dev)
                self.nbr_sims = torch.empty(shape, dtype=torch.float32, device=self.dev)
                ws = torch.empty(max(neighbour_bytes(self.n_entities, self.stored)[1], 4),
                                 dtype=torch.uint8, device=self.dev)
                _lib.call("mf_cf_neighbours", *lists, self.stored, _tp(ws), _tp(self.nbr_ids),
                          _tp(self.nbr_sims), self.stream)
                self.synchronize()                    # the workspace is freed here

    def _fn(self, name: str) -> str:
        return name if self.stored is None else name + "_nbr"

    def _sim_args(self) -> tuple:
        """The similarity operand of the prediction entry points."""
        if self.stored is None:
            return (_tp(self.S),)
        return _tp(self.nbr_ids), _tp(self.nbr_sims), self.stored

    @property
    def stream(self):
        return _VOID(torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def _csr(major, minor, r, n_major, n_minor):
        """(int64 offsets, int32 minor ids, float32 ratings) sorted by (major,
        minor), built on the device."""
        order = torch.argsort(major * max(n_minor, 1) + minor)
        ptr = torch.zeros(n_major + 1, dtype=torch.int64, device=major.device)
        if major.numel():
            torch.cumsum(torch.bincount(major, minlength=n_major), 0, out=ptr[1:])
        return ptr, minor[order].to(torch.int32).contiguous(), r[order].contiguous()

    def synchronize(self) -> None:
        torch.cuda.current_stream(self.dev).synchronize()

    def predict(self, ent: np.ndarray, oth: np.ndarray, n_neighbors: int, global_mean: float,
                min_rating: float, max_rating: float, bound: bool) -> np.ndarray:
        """FP64 predictions for the pairs (ent[p], oth[p]); -1 = unknown id."""
        n = len(ent)
        out = torch.empty(n, dtype=torch.float64, device=self.dev)
        optr, oent, orr = self.other_csr
        with torch.cuda.device(self.dev):
            d_e = torch.from_numpy(np.ascontiguousarray(ent, dtype=np.int32)).to(self.dev)
            d_o = torch.from_numpy(np.ascontiguousarray(oth, dtype=np.int32)).to(self.dev)
            for c0 in range(0, n, PREDICT_CHUNK):
                m = min(PREDICT_CHUNK, n - c0)
                _lib.call(self._fn("mf_cf_predict"), _VOID(d_e.data_ptr() + 4 * c0),
                          _VOID(d_o.data_ptr() + 4 * c0), m, _tp(optr), _tp(oent), _tp(orr),
                          *self._sim_args(), _tp(self.mean), self.n_entities, self.n_others,
                          _lib.MF_F32, int(n_neighbors), float(global_mean), float(min_rating),
                          float(max_rating), int(bool(bound)), _VOID(out.data_ptr() + 8 * c0),
                          self.stream)
        return out.cpu().numpy()

    # ------------------------------------------- one query against every target
    # key workspace of one mf_cf_topk / mf_cf_rank launch (8 B per query and
    # target); queries beyond this budget go in further launches
    topk_ws_budget = 1 << 30
    # targets a workgroup of k_cf_scores walks (0: the library's choice)
    targets_per_block = 0

    def n_targets(self, side: int) -> int:
        return self.n_entities if side == _lib.MF_CF_QUERY_OTHER else self.n_others

    def _query_chunk(self, side: int) -> int:
        """Queries per launch: the key workspace within ``topk_ws_budget`` and
        the grid (one workgroup per query and block of targets) within 2^31 - 1."""
        nt = self.n_targets(side)
        if nt == 0:
            return 1 << 20
        tpb = _lib.load().mf_cf_targets_per_block(nt, int(self.targets_per_block))
        blocks = (nt + tpb - 1) // tpb
        return max(1, min(int(self.topk_ws_budget) // (8 * nt), (2**31 - 1) // blocks))

    def _model_args(self, n_neighbors: int, global_mean: float) -> tuple:
        optr, oent, orr = self.other_csr
        return (_tp(optr), _tp(oent), _tp(orr), *self._sim_args(), _tp(self.mean), self.n_entities,
                self.n_others, _lib.MF_F32, int(n_neighbors), float(global_mean),
                int(self.targets_per_block))

    def _to(self, a, dtype) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def _exclusions(self, nq: int, ex_ptr, ex_items):
        """The exclusion CSR on the device (offsets from 0), or (None, None)."""
        # (mf_cf_topk / mf_cf_rank take the lists in any order)
        ex_ptr, ex_items = exclusion_csr(nq, ex_ptr, ex_items, sort=False)
        if ex_ptr is None:
            return None, None
        return self._to(ex_ptr, np.int64), self._to(ex_items, np.int32)

    def scores(self, queries: np.ndarray, side: int, n_neighbors: int,
               global_mean: float) -> np.ndarray:
        """FP64 scores [n_query, n_targets] of every target for each query id
        (mf_cf_scores): ``predict(bound=False)`` of the corresponding pairs, bit
        for bit.  side: _lib.MF_CF_QUERY_OTHER (queries are other ids, targets
        the entities) or MF_CF_QUERY_ENTITY (queries are entity ids, targets
        the others); -1 = unknown id."""
        nq, nt = len(queries), self.n_targets(side)
        out = torch.empty((nq, nt), dtype=torch.float64, device=self.dev)
        if nq and nt:
            chunk = self._query_chunk(side)
            with torch.cuda.device(self.dev):
                d_q = self._to(queries, np.int32)
                for q0 in range(0, nq, chunk):
                    m = min(chunk, nq - q0)
                    _lib.call(self._fn("mf_cf_scores"), _VOID(d_q.data_ptr() + 4 * q0), m, int(side),
                              *self._model_args(n_neighbors, global_mean),
                              _VOID(out.data_ptr() + 8 * nt * q0), self.stream)
        return out.cpu().numpy()

    def topk(self, queries: np.ndarray, side: int, n_neighbors: int, global_mean: float,
             amount: int, ex_ptr=None, ex_items=None):
        """Best ``amount`` targets per query (mf_cf_topk): (target ids int32
        [n_query, amount], scores float64), score descending then id ascending,
        padded with -1 / NaN.  ``ex_ptr`` / ``ex_items``: optional CSR
        exclusions (query q skips targets ex_items[ex_ptr[q]:ex_ptr[q+1]])."""
        nq, nt, amount = len(queries), self.n_targets(side), int(amount)
        if nq == 0 or amount == 0:
            return (np.full((nq, amount), -1, np.int32),
                    np.full((nq, amount), np.nan, np.float64))
        items = torch.empty((nq, amount), dtype=torch.int32, device=self.dev)
        scores = torch.empty((nq, amount), dtype=torch.float64, device=self.dev)
        chunk = min(nq, self._query_chunk(side))
        with torch.cuda.device(self.dev):
            d_q = self._to(queries, np.int32)
            d_ptr, d_ex = self._exclusions(nq, ex_ptr, ex_items)
            ws = torch.empty(max(8 * chunk * nt, 8), dtype=torch.uint8, device=self.dev)
            for q0 in range(0, nq, chunk):
                m = min(chunk, nq - q0)
                # CSR offsets stay absolute: the chunk's ptr array starts at row q0
                dp = None if d_ptr is None else _VOID(d_ptr.data_ptr() + 8 * q0)
                _lib.call(self._fn("mf_cf_topk"), _VOID(d_q.data_ptr() + 4 * q0), m, int(side),
                          *self._model_args(n_neighbors, global_mean), dp, _tp(d_ex), amount,
                          _tp(ws), _VOID(items.data_ptr() + 4 * amount * q0),
                          _VOID(scores.data_ptr() + 8 * amount * q0), self.stream)
        return items.cpu().numpy(), scores.cpu().numpy()

    def rank(self, queries: np.ndarray, side: int, n_neighbors: int, global_mean: float,
             tgt_ptr: np.ndarray, tgt_items: np.ndarray, ex_ptr=None, ex_items=None):
        """Exact rank of each target among its query's candidates (mf_cf_rank):
        (ranks int32[n_targets], n_candidates int32[n_query]), DeviceModel.rank's
        contract: ``tgt_ptr`` / ``tgt_items`` are a CSR of target ids per query
        (any order, repeats allowed); a target out of range or excluded for
        its query gets rank -1."""
        nq, nt = len(queries), self.n_targets(side)
        tgt_ptr, tgt_items, n_tgt = target_csr(nq, tgt_ptr, tgt_items)
        if nq == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        ranks = torch.empty(max(n_tgt, 1), dtype=torch.int32, device=self.dev)
        cands = torch.empty(nq, dtype=torch.int32, device=self.dev)
        chunk = min(nq, self._query_chunk(side))
        with torch.cuda.device(self.dev):
            d_q = self._to(queries, np.int32)
            d_ptr, d_ex = self._exclusions(nq, ex_ptr, ex_items)
            d_tp = self._to(tgt_ptr, np.int64)
            d_ti = self._to(tgt_items if n_tgt else np.zeros(1, np.int32), np.int32)
            ws = torch.empty(max(8 * chunk * nt, 8), dtype=torch.uint8, device=self.dev)
            for q0 in range(0, nq, chunk):
                m = min(chunk, nq - q0)
                # both CSRs keep absolute offsets: their ptr arrays start at row q0
                dp = None if d_ptr is None else _VOID(d_ptr.data_ptr() + 8 * q0)
                _lib.call(self._fn("mf_cf_rank"), _VOID(d_q.data_ptr() + 4 * q0), m, int(side),
                          *self._model_args(n_neighbors, global_mean), dp, _tp(d_ex),
                          _VOID(d_tp.data_ptr() + 8 * q0), _tp(d_ti), _tp(ws), _tp(ranks),
                          _VOID(cands.data_ptr() + 4 * q0), self.stream)
        return ranks[:n_tgt].cpu().numpy(), cands.cpu().numpy()
