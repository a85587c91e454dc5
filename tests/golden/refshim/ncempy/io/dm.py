"""`fileDM` of a .gtg file without scan geometry: an empty tag set, whatever the path (the synthetic K2IS sets
have no .gtg beside them), so the reference loads them as time series."""


class fileDM:
    def __init__(self, filename, verbose=False, on_memory=False):
        self.filename = filename
        self.allTags = {}

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        return False
