from .hstu import HSTUModel  # noqa: F401
