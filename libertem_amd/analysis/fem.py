"""Fluctuation EM (reference analysis/fem.py:49-68): FEMUDF, the std of a ring in every frame."""
from libertem_amd.udf.FEM import FEMUDF
from .base import BaseAnalysis, AnalysisResult, AnalysisResultSet


class FEMAnalysis(BaseAnalysis, id_="FEM"):
    TYPE = 'UDF'

    def get_udf(self):
        # parameters cx, cy, ri, ro; the UDF takes the center as (row, column) (analysis/fem.py:52-56)
        center = (self.parameters["cy"], self.parameters["cx"])
        return FEMUDF(center=center, rad_in=self.parameters["ri"], rad_out=self.parameters["ro"])

    def get_udf_results(self, udf_results, roi, damage):
        return AnalysisResultSet([
            AnalysisResult(raw_data=udf_results['intensity'].data, key="intensity", title="intensity",
                           desc="result from SD calculation over ring"),
        ])
