from . import dm  # noqa
