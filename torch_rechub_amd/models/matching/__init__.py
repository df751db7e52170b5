"""Matching models on the hot path: DSSM (config 5), its pair-wise (FaceBookDSSM), sampling-bias-corrected (YoutubeSBC) and
SENET-gated (DSSMSENet: the reference's ``dssm_senet.DSSM``) relatives, the list-wise retrieval models YoutubeDNN, MIND,
ComirecSA and ComirecDR, the session-based NARM, STAMP and GRU4Rec, SINE and SASRec (reference
torch_rechub/models/matching/)."""
from .comirec import ComirecDR, ComirecSA
from .dssm import DSSM
from .dssm_facebook import FaceBookDSSM
from .dssm_senet import DSSM as DSSMSENet
from .gru4rec import GRU4Rec
from .mind import MIND
from .narm import NARM
from .sasrec import SASRec
from .sine import SINE
from .stamp import STAMP
from .youtube_dnn import YoutubeDNN
from .youtube_sbc import YoutubeSBC

__all__ = ["DSSM", "FaceBookDSSM", "YoutubeSBC", "DSSMSENet", "YoutubeDNN", "MIND", "ComirecSA", "ComirecDR", "NARM", "STAMP",
           "GRU4Rec", "SINE", "SASRec"]
