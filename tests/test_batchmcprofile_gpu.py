"""Renderer "batchmcprofile" end to end (tools/batchmcprofile.py's run()): a five-thickness sweep of the C4
layers. The table's Monte-Carlo columns are ctx.mc_profile's totals per thickness at the six digits written,
its multipole columns mpss.mc_reference's (the host code, desiredLength 1024) at rtol 1e-5, the tolerance
test_render_writes_reference_file uses for the same comparison."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = """Renderer "batchmcprofile"
  "layer layers" [ 723.6646118164062 577.9549560546875 1.399999976158142 0.0024999999441206455 9.664658546447754 288.97747802734375 1.399999976158142 0.20000000298023224 ]
  "float mfprange" 16
  "integer segments" 64
  "float thicknessrange" [ 0.0001 0.005 ]
  "integer thicknesssegments" 4
  "string photons" "50000"
  "string filename" "sweep.txt"
WorldBegin
WorldEnd
"""


def test_tool_writes_the_table(mpss, tmp_path):
    import torch
    assert torch.cuda.is_available()
    from mpss import batchmcprofile
    spec = importlib.util.spec_from_file_location("batchmcprofile_tool", os.path.join(ROOT, "tools", "batchmcprofile.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    scene = tmp_path / "sweep.pbrt"
    scene.write_text(SCENE)
    r, path = tool.run(str(scene))
    assert path == str(tmp_path / "sweep.txt")  # "filename" is relative to the scene file
    lines = open(path).read().split("\n")
    assert lines[0] == batchmcprofile.HEADER and len(lines) == 7 and lines[6] == ""
    rows = batchmcprofile.read_tsv(path)
    th = r.thicknesses()
    assert len(rows) == 5 and [row["thickness"] for row in rows] == [float("%g" % t) for t in th]
    assert np.all(np.diff([row["thickness"] for row in rows]) > 0)
    assert len(r.results) == 5
    for row, res in zip(rows, r.results):
        assert sorted(row) == sorted(res)
        for k in res:
            assert row[k] == float("%g" % res[k])
    ctx = mpss.Context()
    for row, lay in zip(rows, r.slabs()):
        mc = ctx.mc_profile(lay, 16.0, 64, 50000, seed=89)
        assert "%g" % row["totalMCReflectance"] == "%g" % mc["total_r"]
        assert "%g" % row["totalMCTransmittance"] == "%g" % mc["total_t"]
        for lerp, name in ((False, "NoLerp"), (True, "Lerp")):
            ref = mpss.mc_reference(lay, 16.0, 64, lerp)
            assert row["total%sReflectance" % name] == pytest.approx(ref["total_r"], rel=1e-5)
            assert row["total%sTransmittance" % name] == pytest.approx(ref["total_t"], rel=1e-5)
    ctx.close()
