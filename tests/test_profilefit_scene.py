"""Renderer "multipoleprofilefit" through the scene loader and tools/profilefit.py's pieces, on the CPU; and the
GPU tests' precondition that the host fit's choice of window is rarely a near-tie on their inputs."""
import io

import numpy as np
import pytest

import sog_ref


def test_scene_description_and_host_run(mpss, tmp_path):
    from mpss import pbrtscene, profilefit
    scene = tmp_path / "fit.pbrt"
    scene.write_text('Renderer "multipoleprofilefit" "float f_mel" [ 0.1 0.01 ] "float f_eu" [ 0.5 ]\n'
                     '  "float f_blood" [ 0.002 ] "float f_ohg" [ 0.9 0.3 ] "skinlayer layers" [ 0.25e6 1.4 20e6 1.4 ]\n'
                     '  "string filename" "out.txt" "integer desiredProfileLength" 16 "integer idrange" [ 1 3 ]\n'
                     'WorldBegin\nWorldEnd\n')
    sc = pbrtscene.load(str(scene))
    kind, d = sc.renderer
    assert kind == "multipoleprofilefit"
    assert d["ranges"]["f_mel"] == [0.01, 0.1] and d["ranges"]["f_ohg"] == [0.3, 0.9]  # sorted, as FindParamRange
    assert d["layers"] == [(0.25e6, 1.4), (20e6, 1.4)] and d["desired_length"] == 16 and d["id_range"] == (1, 3)
    assert d["filename"] == str(tmp_path / "out.txt")
    res, id_min = profilefit.run(d["ranges"], d["layers"], d["desired_length"], d["id_range"])
    assert id_min == 1 and res["coeffs"].shape[0] == 2
    buf = io.StringIO()
    profilefit.write_table(buf, d["ranges"], res, id_min)
    assert buf.getvalue().startswith("1\t0.01\t0.5\t0.002\t0.9\t405\t")  # no header: the range starts at id 1


def test_defaults_and_refusals(mpss, tmp_path):
    from mpss import pbrtscene
    scene = tmp_path / "fit.pbrt"
    body = ('"float f_mel" [ 0.1 ] "float f_eu" [ 0.5 ] "float f_blood" [ 0.002 ] "float f_ohg" [ 0.3 ] '
            '"skinlayer layers" [ 0.25e6 1.4 20e6 1.4 ]')
    scene.write_text('Renderer "multipoleprofilefit" %s\nWorldBegin\nWorldEnd\n' % body)
    d = pbrtscene.load(str(scene)).renderer[1]
    assert d["desired_length"] == 256 and d["id_range"] == (0, -1) and d["filename"] == ""
    scene.write_text('Renderer "multipoleprofilefit" %s "integer splittasks" 4\nWorldBegin\nWorldEnd\n' % body)
    with pytest.raises(ValueError, match="splittasks.*not built"):
        pbrtscene.load(str(scene))
    scene.write_text('Renderer "multipoleprofilefit" "float f_mel" [ 0.1 ]\nWorldBegin\nWorldEnd\n')
    with pytest.raises(ValueError, match="f_eu not specified"):
        pbrtscene.load(str(scene))
    f = mpss.profile_fit_spec([0.1], [0.5], [0.002], [0.3])[0]
    assert (f.desired_length, f.id_min, f.id_max, f.max_profiles_per_batch) == (256, 0, -1, 0)


def test_shipped_scene_loads(mpss):
    import os
    from mpss import pbrtscene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = pbrtscene.load(os.path.join(root, "scenes", "profilefit.pbrt")).renderer[1]
    assert len(d["ranges"]["f_mel"]) * len(d["ranges"]["f_blood"]) * len(d["ranges"]["f_ohg"]) == 12


@pytest.mark.parametrize("dl", (16, 64))
def test_host_choice_is_rarely_a_near_tie(mpss, dl):
    """the GPU tests leave near-ties (best and second-best error within 1e-5 relative) out of the centre
    comparison; on their inputs the host fit alone must keep those under 2 %"""
    case = sog_ref.grid_case(mpss, dl)
    amb = sog_ref.ambiguous(case["sog"]["cand_error"])
    assert amb.mean() <= 0.02, int(amb.sum())
    assert (case["sog"]["centre"] >= 3).all()
