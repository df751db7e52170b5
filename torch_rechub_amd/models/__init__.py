from . import generative, matching, ranking  # noqa: F401
