from . import activation, callback, features, initializers, layers, loss_func, metric  # noqa: F401
