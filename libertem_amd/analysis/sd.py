"""Standard deviation of all frames (reference analysis/sd.py:56-97): StdDevUDF per pixel."""
from libertem_amd.udf.stddev import StdDevUDF
from .base import BaseAnalysis, AnalysisResult, AnalysisResultSet
from .getroi import get_roi


class SDAnalysis(BaseAnalysis, id_="SD_FRAMES"):
    TYPE = 'UDF'

    def get_udf(self):
        return StdDevUDF()

    def get_roi(self):
        # parameters = {'roi': {'shape': 'disk' | 'rect', ...}} (analysis/sd.py:62-63)
        return get_roi(params=self.parameters, shape=self.dataset.shape.nav)

    def get_udf_results(self, udf_results, roi, damage):
        std = udf_results['std'].data
        return AnalysisResultSet([
            AnalysisResult(raw_data=std, key="intensity", title="intensity [log]",
                           desc="Standard deviation of frames log-scaled"),
            AnalysisResult(raw_data=std, key="intensity_lin", title="intensity [lin]",
                           desc="Standard deviation of frames lin-scaled"),
        ])
