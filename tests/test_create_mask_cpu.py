"""create_mask drop-in without a GPU: the answer scripts the reference produces (tests/golden/create_mask_scripts.json), every refusal,
the float64 restatement (tests/f64_create_mask.py) against what is known by construction and against its second labeller, the gap
condition that lets tests/test_gpu_create_mask.py demand equality after a float32 transform, and cli.create_mask_main with a float64
backend."""
import ctypes
import io
import json
import os
import subprocess

import numpy as np
import pytest

import f64_create_mask as CM
import f64_mask as FM
from pyp_amd.abi import CreateMaskCfg, CreateMaskInfo
from pyp_amd.formats import mrc
from pyp_amd.surface import cli, prompts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCRIPTS = json.load(open(os.path.join(GOLDEN, "create_mask_scripts.json")))["scripts"]

EIGHT = ["ref.mrc", "mask.mrc", "1.7", "200", "No", "0.84", "10.0", "0.35"]


# ------------------------------------------------------------------------------------------ answers
@pytest.mark.parametrize("case", SCRIPTS, ids=[c["case"] for c in SCRIPTS])
def test_parse_reference_scripts(case):
    header, script, alter, apply_script = case["commands"]
    assert header.startswith("/opt/imod/bin/header -pixel") and alter.startswith("/opt/imod/bin/alterheader -del")
    prog, log, answers = prompts.split_heredoc(script)
    assert prog == "/opt/pyp/external/frealignx/create_mask" and log == "/dev/null"
    d = prompts.parse_create_mask(answers)
    p = case["parameters"]
    assert d["input"].endswith("t20s_r01_02.mrc")                       # a `_crop.mrc` model: the full map is what is masked
    assert d["output"] == "frealign/maps/mask.mrc" and d["output"] in alter
    assert d["pixel_size"] == case["pixel_size"] and d["outer_radius"] == p["particle_rad"]
    assert d["auto_threshold"] is False and d["rebin"] == 0.35 and d["lowpass"] == p["mask_lowpass"]
    if p.get("mask_normalized"):
        assert d["threshold"] != p["mask_threshold"]                    # min + fraction x (max - min) of the `_crop.mrc` twin
    else:
        assert d["threshold"] == p["mask_threshold"]
    a = prompts.parse_apply_mask(prompts.split_heredoc(apply_script)[2])
    assert a["mask"] == d["output"] and a["output"] == case["output"] and a["map"] == os.path.basename(d["input"])
    assert a["edge_width"] == p["mask_edge_width"] and a["outside_weight"] == p["mask_outside_weight"]


def test_fixture_covers_the_cases():
    tags = {c["case"] for c in SCRIPTS}
    assert {"normalized_threshold", "absolute_threshold", "crop_model"} <= tags
    assert len({c["parameters"]["mask_lowpass"] for c in SCRIPTS}) >= 2
    crop = [c for c in SCRIPTS if c["case"] == "crop_model"][0]
    assert crop["model"].endswith("_crop.mrc") and "_crop" not in crop["commands"][1]


def test_parse_the_docstring_defaults():
    d = prompts.parse_create_mask(EIGHT)
    assert d == dict(input="ref.mrc", output="mask.mrc", pixel_size=1.7, outer_radius=200.0, auto_threshold=False, threshold=0.84,
                     lowpass=10.0, rebin=0.35)
    assert prompts.parse_create_mask(EIGHT[:6] + ["0", "7"])["lowpass"] == 0.0          # no low-pass: the re-bin value is not used
    assert prompts.parse_create_mask(EIGHT[:5] + ["-0.2"] + EIGHT[6:])["threshold"] == -0.2
    assert prompts.CREATE_MASK_EDGE_PX == CM.EDGE_PX == 4.0


def _with(i, value, base=EIGHT):
    a = list(base)
    a[i] = value
    return a


@pytest.mark.parametrize("answers, word", [
    (_with(4, "Yes"), "automatic"), (_with(4, "maybe"), "yes or no"),
    (_with(7, "0"), "re-bin"), (_with(7, "-0.1"), "re-bin"), (_with(7, "1"), "re-bin"), (_with(7, "1.5"), "re-bin"),
    (_with(6, "-10"), "low-pass"), (_with(2, "0"), "pixel"), (_with(2, "-1.7"), "pixel"), (_with(3, "0"), "radius"),
    (_with(3, "-200"), "radius"), (_with(5, "abc"), "number"), (_with(5, "nan"), "threshold"), (_with(0, ""), "empty"),
    (EIGHT[:7], "answers"), (EIGHT + ["extra"], "answers"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_parse_refusals(answers, word):
    with pytest.raises(prompts.PromptError) as e:
        prompts.parse_create_mask(answers)
    assert str(e.value).startswith("ERROR: ") and word in str(e.value)


# ------------------------------------------------------------------------------------------ the float64 restatement against itself
@pytest.mark.parametrize("name", CM.CASES)
@pytest.mark.parametrize("n", [8, 31, 65])
def test_model_on_crafted_bodies(n, name):
    vol, radius, known = CM.crafted(name, n)
    mask, info = CM.create_mask(vol, 1.0, radius, 0.5)
    for k, v in known.items():
        if k != "first":
            assert info[k] == v, (k, info[k], v)
    if "first" in known:
        assert int(np.argmax(mask.reshape(-1))) == known["first"]
    assert info["mask_voxels"] == info["largest"] == int(mask.sum()) and info["above"] >= info["largest"]
    assert (mask.astype(bool) <= (vol >= 0.5)).all()
    if CM._ndimage is not None:                                           # the two labellers
        mask2, info2 = CM.create_mask(vol, 1.0, radius, 0.5, labeller=CM.label_runs)
        assert np.array_equal(mask, mask2)
        assert all(info[k] == info2[k] for k in ("above", "components", "largest", "mask_voxels"))


def test_model_connectivity_and_faces():
    n = 8
    vol, radius, _ = CM.crafted("corner_touch", n)
    lab6 = None if CM._ndimage is None else CM._ndimage.label(vol >= 0.5)[1]
    assert lab6 in (None, 3)                                              # two cubes and a bar at 6-connectivity, ...
    assert CM.create_mask(vol, 1.0, radius, 0.5)[1]["components"] == 2    # ... cubes joined through their corner at 26
    vol, radius, _ = CM.crafted("opposite_faces", n)
    assert CM.create_mask(vol, 1.0, radius, 0.5)[1]["components"] == 2    # no wrap-around


def test_model_refuses_an_empty_threshold():
    vol, radius, _ = CM.crafted("equal_bodies", 8)
    with pytest.raises(CM.Refused, match="ranges from 0 to 1"):
        CM.create_mask(vol, 1.0, radius, 1.5)
    vol, radius, _ = CM.crafted("outside_sphere", 8)
    mask, info = CM.create_mask(vol, 1.0, radius, 0.5)
    assert info["above"] == 8 and not mask[0].any()                        # the sphere is applied before the labelling


def test_sphere_is_integer():
    s = CM.sphere(8, 3.0, 1.0)
    assert s[4, 4, 7] and s[4, 4, 1] and not s[4, 4, 0] and not s[4, 5, 7] and s.sum() == 123       # lattice points with d^2 <= 9
    assert np.array_equal(CM.sphere(8, 6.0, 2.0), s) and CM.sphere(31, 1000.0, 1.0).all()


def test_pick_threshold():
    t, gap = CM.pick_threshold([0.0, 0.1, 0.4, 0.45, 1.0], 0.05, 0.5, 0.05)
    assert abs(t - 0.25) < 1e-12 and abs(gap - 6.0) < 1e-9
    with pytest.raises(AssertionError):
        CM.pick_threshold([0.0, 1.0], 0.2, 0.8, 0.1)


@pytest.mark.parametrize("n", [32, 48])
def test_gap_condition(n):
    """What lets the GPU test demand equality: t and b sit in gaps of at least four bands (f64_mask.bound_filtered), so no voxel of L
    (of the low-passed body) lies within two bands of its comparison, while the GPU is held to one.  Widest gaps found with these
    inputs, in bands: 61 (t) and 100 (b) at 32, 17 and 43 at 48."""
    c = CM.lowpass_case(n)
    assert c["t_gap"] >= 4 and c["b_gap"] >= 4, (c["t_gap"], c["b_gap"])
    sph = CM.sphere(n, c["radius_A"], c["pixel"])
    assert np.abs(c["L"][sph] - c["t"]).min() >= 2 * FM.bound_filtered(n, c["L"]) * 0.999
    assert np.abs(c["S"][sph] - c["b"]).min() >= 2 * FM.bound_filtered(n, c["S"]) * 0.999
    mask, info = CM.create_mask(c["vol"], c["pixel"], c["radius_A"], c["t"], c["lowpass_A"], c["edge"], c["b"], L=c["L"])
    assert info["components"] >= 3 and info["largest"] < info["above"]          # several bodies: the selection matters
    assert info["mask_voxels"] > info["largest"]                                # b < 0.5 grows the body
    assert 0.30 <= c["b"] <= 0.40


def test_script_case_has_room():
    """The map of the executables' GPU test: scaled so that the fixture script's own threshold and the fixed re-bin value of 0.35 keep
    two bands from every voxel."""
    case = [c for c in SCRIPTS if c["case"] == "absolute_threshold"][0]
    p = case["parameters"]
    sc = CM.script_case(32, case["pixel_size"], p["particle_rad"], p["mask_lowpass"], p["mask_threshold"], 0.35)
    assert sc["t_room"] >= 2 and sc["b_room"] >= 2, (sc["t_room"], sc["b_room"])
    mask, info = CM.create_mask(sc["vol"], case["pixel_size"], p["particle_rad"], p["mask_threshold"], p["mask_lowpass"], sc["edge"], 0.35, L=sc["L"])
    assert info["components"] >= 1 and info["largest"] < info["mask_voxels"] < 32 ** 3


# ------------------------------------------------------------------------------------------ the structs
def test_structs_match_the_header(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cf = ["pixel_size", "outer_radius_A", "threshold", "lowpass_A", "lowpass_edge_px", "rebin"]
    nf = ["density_min", "density_max", "above", "components", "largest", "mask_voxels"]
    fmt = " ".join(["%zu"] * (2 + len(cf) + len(nf)))
    args = ", ".join(["sizeof(ppm_create_mask_cfg)"] + [f"offsetof(ppm_create_mask_cfg, {f})" for f in cf] +
                     ["sizeof(ppm_create_mask_info)"] + [f"offsetof(ppm_create_mask_info, {f})" for f in nf])
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ppm.h"\nint main(void){ printf("%s\\n", %s); return 0; }\n' % (fmt, args)
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", str(tmp_path / "t"), str(tmp_path / "t.c")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).decode().split()]
    want = ([ctypes.sizeof(CreateMaskCfg)] + [getattr(CreateMaskCfg, f).offset for f in cf] +
            [ctypes.sizeof(CreateMaskInfo)] + [getattr(CreateMaskInfo, f).offset for f in nf])
    assert got == want
    c = CreateMaskCfg.make(1.35, 80, 0.42, lowpass_A=10)
    assert (c.pixel_size, c.outer_radius_A, c.threshold, c.lowpass_A, c.lowpass_edge_px, c.rebin) == (1.35, 80.0, 0.42, 10.0, 4.0, 0.35)


# ------------------------------------------------------------------------------------------ the executable with a float64 backend
def f64_backend(seen):
    def run(vol, cfg):
        seen.append(cfg)
        mask, info = CM.create_mask(vol, cfg.pixel_size, cfg.outer_radius_A, cfg.threshold, cfg.lowpass_A, cfg.lowpass_edge_px, cfg.rebin)
        return mask.astype(np.float32), CreateMaskInfo(**{k: info[k] for k, _ in CreateMaskInfo._fields_})
    return run


def _script_answers(case, tmp_path, threshold=None):
    answers = prompts.split_heredoc(case["commands"][1])[2]
    answers[0], answers[1] = str(tmp_path / "map.mrc"), str(tmp_path / "mask.mrc")
    if threshold is not None:
        answers[5] = repr(threshold)
    return answers


def test_main_writes_the_mask_with_the_pixel_size(tmp_path, capsys):
    n = 32
    vol = CM.lowpass_map(n)
    mrc.write(vol, str(tmp_path / "map.mrc"), pixel_size=2.0)                # the script's pixel size wins over the header's
    case = [c for c in SCRIPTS if c["case"] == "absolute_threshold"][0]
    seen = []
    answers = _script_answers(case, tmp_path, threshold=1.5)
    assert cli.create_mask_main(stdin=io.StringIO("\n".join(answers) + "\n"), backend=f64_backend(seen)) == 0
    out = capsys.readouterr().out
    assert out.rstrip().endswith("CreateMask: Normal termination")
    cfg = seen[0]
    assert (cfg.pixel_size, cfg.outer_radius_A, cfg.threshold, cfg.lowpass_A, cfg.rebin) == (1.35, 80.0, 1.5, 10.0, 0.35)
    assert cfg.lowpass_edge_px == 4.0                                        # r_c = 32 x 1.35 / 10 = 4.3: not clipped
    h = mrc.read_header(str(tmp_path / "mask.mrc"))
    assert h["mode"] == 2 and abs(h["pixel_size"] - 1.35) < 1e-6
    got = mrc.read(str(tmp_path / "mask.mrc"))
    want, info = CM.create_mask(vol, 1.35, 80.0, 1.5, 10.0, 4.0, 0.35)
    assert np.array_equal(got, want.astype(np.float32)) and set(np.unique(got)) <= {0.0, 1.0}
    for word, key in (("Voxels above the threshold", "above"), ("Connected components", "components"), ("Voxels of the largest", "largest"),
                      ("Voxels of the mask", "mask_voxels")):
        line = [ln for ln in out.splitlines() if ln.startswith(word)]
        assert len(line) == 1 and int(line[0].split(":")[1]) == info[key]
    assert "Density inside the radius" in out
    assert sorted(os.listdir(tmp_path)) == ["map.mrc", "mask.mrc"]


def test_main_clips_the_edge_to_twice_the_radius(tmp_path):
    mrc.write(CM.lowpass_map(32), str(tmp_path / "map.mrc"), pixel_size=1.0)
    a = [str(tmp_path / "map.mrc"), str(tmp_path / "mask.mrc"), "1.0", "30", "No", "0.7", "20", "0.35"]      # r_c = 1.6: e = 3.2
    seen = []
    assert cli.create_mask_main(stdin=io.StringIO("\n".join(a) + "\n"), backend=f64_backend(seen)) == 0
    assert abs(seen[0].lowpass_edge_px - 3.2) < 1e-12


def _refused(tmp_path, answers, capsys, backend=None):
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit) as e:
        cli.create_mask_main(stdin=io.StringIO("\n".join(answers) + "\n"), backend=backend or f64_backend([]))
    assert e.value.code != 0
    assert "ERROR" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path)) == before


def test_main_refusals_leave_the_directory_as_it_was(tmp_path, capsys):
    mrc.write(CM.lowpass_map(32), str(tmp_path / "map.mrc"), pixel_size=1.35)
    mrc.write(np.zeros((16, 32, 32), np.float32), str(tmp_path / "slab.mrc"))
    base = [str(tmp_path / "map.mrc"), str(tmp_path / "mask.mrc"), "1.35", "80", "No", "1.5", "10", "0.35"]
    _refused(tmp_path, _with(4, "Yes", base), capsys)
    _refused(tmp_path, _with(7, "1.0", base), capsys)
    _refused(tmp_path, _with(6, "-1", base), capsys)
    _refused(tmp_path, base[:7], capsys)
    _refused(tmp_path, _with(0, str(tmp_path / "absent.mrc"), base), capsys)
    _refused(tmp_path, _with(0, str(tmp_path / "slab.mrc"), base), capsys)              # not cubic
    _refused(tmp_path, _with(5, "1000", base), capsys)                                  # the threshold no voxel reaches
    with pytest.raises(SystemExit):
        cli.create_mask_main(stdin=io.StringIO("\n".join(_with(5, "1000", base)) + "\n"), backend=f64_backend([]))
    assert "ranges from" in capsys.readouterr().out
