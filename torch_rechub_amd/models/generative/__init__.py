from .hstu import HSTUModel  # noqa: F401
from .hllm import HLLMModel, HLLMTransformerBlock  # noqa: F401
from .rqvae import RQVAEModel, ResidualVectorQuantizer, VectorQuantizer  # noqa: F401
from .tiger import TIGERConfig, TIGERModel  # noqa: F401
