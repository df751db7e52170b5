"""Matching models on the hot path: DSSM (config 5) and the list-wise retrieval models YoutubeDNN, MIND, ComirecSA and
ComirecDR, the session-based NARM, STAMP and GRU4Rec, SINE and SASRec (reference torch_rechub/models/matching/)."""
from .comirec import ComirecDR, ComirecSA
from .dssm import DSSM
from .gru4rec import GRU4Rec
from .mind import MIND
from .narm import NARM
from .sasrec import SASRec
from .sine import SINE
from .stamp import STAMP
from .youtube_dnn import YoutubeDNN

__all__ = ["DSSM", "YoutubeDNN", "MIND", "ComirecSA", "ComirecDR", "NARM", "STAMP", "GRU4Rec", "SINE", "SASRec"]
