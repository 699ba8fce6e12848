"""matrix_factorization -- MI355X-native drop-in for the SGD path of
SHEEPididoo/matrix-factorization.

Same public names as the reference package for the path this build covers
(matrix_factorization/__init__.py:1-16 of the reference): KernelMF and
BaselineModel train on the GPU through libmf_hip.so (hand-written gfx950
kernels behind a C ABI, include/mf_hip.h); RecommenderBase and
train_update_test_split are the host-side surface around them.  ALSMF (no
reference counterpart: BASELINE config 5) fits the same linear factor model
by alternating least squares with an MFMA Gramian; ImplicitALSMF (no
reference counterpart either) fits implicit-feedback strengths by
confidence-weighted ALS over all user x item pairs; BPRMF (no counterpart
either) optimises the ranking of each user's positives over the rest by
exact-order SGD on sampled (user, positive, negative) triples.  ItemItemCF and
UserUserCF are the reference's neighbourhood models
(collaborative_filtering.py): a float32 similarity matrix built on the GPU
from the sparse ratings (mf_cf_stats, mf_cf_similarity) and a
top-n_neighbors weighted prediction (mf_cf_predict); with
``stored_neighbors=M`` each entity's M best neighbours in place of the matrix
(mf_cf_neighbours, mf_cf_*_nbr), for entity counts whose matrix does not fit.
ContentBasedRecommender is the reference's content-based model
(content_based.py): rating-weighted feature profiles and the item x item
feature cosine built on the GPU (mf_content_profiles, mf_content_normalize,
mf_content_similarity), the reference's placeholder prediction by default and
two opt-in scorings (cosine retrieval through mf_predict / mf_topk / mf_rank,
similarity-weighted prediction through the mf_cf_* kernels).
HybridRecommender is the path the reference's project_template ships
(pipeline/evaluate_hybrid.py): candidates retrieved by embedding cosine
(profiles and mf_topk as above), then filtered, scored by a fitted factor model
and blended with the cosine in one pass per user (mf_hybrid_rerank).
"""

from .als_matrix_factorization import ALSMF
from .baseline_model import BaselineModel
from .bpr_matrix_factorization import BPRMF
from .collaborative_filtering import ItemItemCF, UserUserCF
from .content_based import ContentBasedRecommender
from .hybrid import HybridRecommender
from .implicit_als_matrix_factorization import ImplicitALSMF
from .kernel_matrix_factorization import KernelMF
from .recommender_base import RecommenderBase
from .utils import ranking_metrics_from_ranks, train_update_test_split

__all__ = [
    "ALSMF",
    "BPRMF",
    "BaselineModel",
    "ContentBasedRecommender",
    "HybridRecommender",
    "ImplicitALSMF",
    "ItemItemCF",
    "KernelMF",
    "RecommenderBase",
    "UserUserCF",
    "ranking_metrics_from_ranks",
    "train_update_test_split",
]

__version__ = "0.1.0"
