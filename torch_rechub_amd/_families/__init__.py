"""The Python side of the stateless leaf kernel families, one module per ``csrc/<name>.hip``.  Each imports ``_lib``,
``_opcore`` and at most a sibling, never ``ops``; ``ops`` re-exports their public names, and callers use ``ops.<name>``."""
