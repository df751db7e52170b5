"""Matching models on the hot path: DSSM (config 5) and the list-wise retrieval models YoutubeDNN, MIND, ComirecSA and
ComirecDR (reference torch_rechub/models/matching/)."""
from .comirec import ComirecDR, ComirecSA
from .dssm import DSSM
from .mind import MIND
from .youtube_dnn import YoutubeDNN

__all__ = ["DSSM", "YoutubeDNN", "MIND", "ComirecSA", "ComirecDR"]
