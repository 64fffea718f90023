from .criteo import CRITEO_FIELD_VOCABS, N_DENSE, N_SPARSE, synthetic_batch
from .ctr import CIN, DCN, DLRM, LR, MODELS, WDL, DeepFM, xDeepFM

__all__ = ["CRITEO_FIELD_VOCABS", "N_DENSE", "N_SPARSE", "synthetic_batch",
           "CIN", "DCN", "DLRM", "LR", "MODELS", "WDL", "DeepFM", "xDeepFM"]
