"""Throw-away stand-in for `ncempy` (absent): only what the reference's K2IS reader imports.  Only for
golden-vector generation."""
