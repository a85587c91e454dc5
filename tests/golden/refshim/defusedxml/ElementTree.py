"""`defusedxml.ElementTree` forwarded to the standard library (the inputs are the generator's own files)."""
from xml.etree.ElementTree import parse, fromstring, iterparse, tostring, ParseError  # noqa: F401
