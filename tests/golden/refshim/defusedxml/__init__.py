"""Throw-away stand-in for `defusedxml` (absent): the standard library's parser under its name, for the
synthetic XML side files of the SEQ and EMPAD sets.  Only for golden-vector generation."""
