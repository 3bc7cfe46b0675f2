from .nav import inflation_lut  # noqa: F401
