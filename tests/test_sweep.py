"""The pigment-sweep plumbing that needs no GPU: the csv reader, the H, M, E, B -> LayeredSkin mapping
of the fork's SceneMaker.py, the command-line tool's options, and the new C entry points."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSV = os.path.join(ROOT, "tests", "golden", "perms_first16.csv")


def test_fixture_rows_and_pigment_mapping(mpss):
    from mpss import sweep
    rows = sweep.read_rows(CSV)
    assert len(rows) == 16 and all(len(r) == 4 for r in rows)
    assert rows[0] == (0.0, 0.055296, 0.28, 0.75) and rows[13] == (0.0, 0.087808, 0.21, 0.5)
    assert sweep.read_rows(CSV, limit=3) == rows[:3]
    # SceneMaker.py:40-51: "skinlayer layers" [E e6 1.4 20e6 1.4], f_mel M, f_eu B, f_blood H
    base = dict(roughness=0.35, nmperunit=40e6, f_ohg=0.75, layer_thickness_nm=[0.25e6, 20e6], layer_ior=[1.4, 1.4],
                Kr=[0.0, 0.0, 0.0], Kt=[0.0, 0.0, 0.0])
    H, M, E, B = rows[13]
    m = sweep.pigment_skin(base, H, M, E, B)
    assert (m["f_blood"], m["f_mel"], m["f_eu"]) == (H, M, B)
    assert m["layer_thickness_nm"] == [pytest.approx(0.21e6), 20e6] and m["layer_ior"] == [1.4, 1.4]
    assert (m["roughness"], m["nmperunit"], m["f_ohg"], m["Kr"]) == (0.35, 40e6, 0.75, [0.0, 0.0, 0.0])
    assert base["layer_thickness_nm"] == [0.25e6, 20e6] and "f_mel" not in base  # the base is not touched
    from mpss import pbrtscene
    s = pbrtscene.skin_struct(m)
    assert (s.f_blood, s.f_mel, s.f_eu) == pytest.approx((H, M, B))
    assert list(s.layer_thickness_nm) == pytest.approx([0.21e6, 20e6]) and list(s.Kr) == [0.0] * 30


def test_csv_reader_skips_empty_cells(mpss, tmp_path):
    """The fork's sampling tables pad their shorter columns with empty cells
    (PigmentSamplingValuesWThickness.csv, with a byte-order mark); such rows are dropped."""
    from mpss import sweep
    p = tmp_path / "pad.csv"
    p.write_bytes(b"\xef\xbb\xbfH,M,E,B\r\n0,0,0.03,0\r\n4.00E-06,4.00E-06,0.04,0.25\r\n0.119164,0.119164,,\r\n"
                  b"0.131072,0.131072, ,\r\n0.5,0.5,0.33,1\r\n")
    assert sweep.read_rows(str(p)) == [(0.0, 0.0, 0.03, 0.0), (4e-6, 4e-6, 0.04, 0.25), (0.5, 0.5, 0.33, 1.0)]
    # columns are found by name, wherever they stand
    p.write_text("B,x,E,M,H\n1,9,0.2,0.1,0.3\n")
    assert sweep.read_rows(str(p)) == [(0.3, 0.1, 0.2, 1.0)]


def test_sweep_tool_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sweep.py"), "--help"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    for opt in ("--out", "--limit", "--mode", "--format", "update", "fresh", "pfm", "exr"):
        assert opt in r.stdout


def test_new_entry_points_are_declared_and_exported(mpss):
    declared = mpss.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", mpss.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("mpss_update_layeredskin", "mpss_build_counts", "mpss_get_common_grid", "mpss_set_grid_builder"):
        assert name in declared and name in exported, name
    assert mpss.lib().mpss_abi_version() == 13  # new entry points only: clients detect them by symbol
    assert mpss.lib().mpss_update_layeredskin(None, 0, None) == -1
    assert mpss.lib().mpss_build_counts(None, None) == -1
