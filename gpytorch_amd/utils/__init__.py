"""Helpers that live under ``gpytorch.utils`` in the reference."""
from . import grid  # noqa: F401
