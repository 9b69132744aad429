from .corr import CorrBlock1D  # noqa: F401
