from . import data, hstu_utils, match  # noqa: F401
