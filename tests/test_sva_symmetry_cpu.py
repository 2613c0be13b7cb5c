"""Point-group symmetry on the sub-tomogram path, the parts a CPU can check: the global search's rotation grid cut to the asymmetric
unit (sva_rotation_grid, pyp_amd/csrc/ppm_geom.h, compiled against the header), the size of ppm_sva_cfg against its ctypes mirror, and the
protocol field `<section>_use_symmetrization` (sva.cfg_from_xml)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from pyp_amd import synth
from pyp_amd.abi import SvaCfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["C2", "C4", "C6", "C7", "D2", "D3", "D7", "T", "O", "I"]
STEPS = [20.0, 30.0]

GRID_SRC = r'''
#include <cstdio>
#include <cstdlib>
#include "ppm_geom.h"
int main(int argc, char **argv) {          // <step> <symbol> pairs -> per pair: the number of rotations, then nine numbers a line
    for (int a = 1; a + 1 < argc; a += 2) {
        const std::vector<double> g = ppm::sva_rotation_grid(std::atof(argv[a]), argv[a + 1]);
        printf("%zu\n", g.size() / 9);
        for (size_t i = 0; i < g.size(); i += 9) {
            for (int k = 0; k < 9; k++) printf("%a ", g[i + k]);
            printf("\n");
        }
    }
    return 0;
}
'''

SIZE_SRC = r'''
#include <cstdio>
#include "ppm.h"
int main() { printf("%zu\n", sizeof(ppm_sva_cfg)); return 0; }
'''


def sym_limits(sym):
    """Restatement of ppm_geom.h's sym_limits: (phi_max, theta_max) of the asymmetric unit."""
    if not sym:
        return 360.0, 180.0
    t, n = sym[0].upper(), int(sym[1:] or 0)
    if t == "C" and n >= 1:
        return 360.0 / n, 180.0
    if t == "D" and n >= 1:
        return 360.0 / n, 90.0
    if t in "TI":
        return 180.0, 90.0
    if t == "O":
        return 90.0, 90.0
    return 360.0, 180.0


def grid_restated(step, sym):
    """The grid of include/ppm.h, ppm_sva_cfg.search_mode 1 / symmetry: with ("", "C1") today's full grid, operand for operand."""
    phi_max, theta_max = sym_limits(sym)
    n_theta = max(2, int(math.floor(theta_max / step + 0.5)) + 1)
    n_psi = max(1, int(math.floor(360.0 / step + 0.5)))
    out = []
    for i in range(n_theta):
        th = theta_max * i / (n_theta - 1)
        n_phi = max(1, int(math.floor(phi_max * math.sin(th * math.pi / 180.0) / step + 0.5)))
        for j in range(n_phi):
            for k in range(n_psi):
                out.append(synth.euler_matrix(k * 360.0 / n_psi, th, phi_max * j / n_phi))
    return np.array(out)


@pytest.fixture(scope="module")
def grids(tmp_path_factory):
    """{(step, symbol): (n, 3, 3)} from the compiled header, for "", C1 and every symbol of the coverage test."""
    d = tmp_path_factory.mktemp("svagrid")
    (d / "g.cpp").write_text(GRID_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "pyp_amd", "csrc"), "-o", str(d / "g"), str(d / "g.cpp")])
    keys = [(s, y) for s in STEPS for y in ["", "C1"] + SYMBOLS]
    args = [x for s, y in keys for x in (repr(s), y)]
    tok = subprocess.check_output([str(d / "g")] + args).decode().split()
    out, at = {}, 0
    for key in keys:
        n = int(tok[at]); at += 1
        out[key] = np.array([float.fromhex(t) for t in tok[at:at + 9 * n]]).reshape(n, 3, 3)
        at += 9 * n
    assert at == len(tok)
    return out


def test_c1_grid_is_todays_grid(grids):
    for step, size in ((20.0, 1908), (30.0, 552)):
        want = grid_restated(step, "")
        assert len(want) == size
        for sym in ("", "C1"):
            got = grids[(step, sym)]
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12, (step, sym)


def test_restricted_grid_sizes_match_the_restatement(grids):
    for step in STEPS:
        for sym in SYMBOLS:
            want = grid_restated(step, sym)
            got = grids[(step, sym)]
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12, (step, sym)
    assert [len(grids[(20.0, s)]) for s in ("C4", "C6", "D7")] == [504, 360, 198]


def random_rotations(n, seed):
    q = np.random.default_rng(seed).normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def nearest_deg(R, ops, G):
    """Per rotation of R: the angle to the nearest S G over operators S and grid rotations G, degrees."""
    A = np.einsum("sji,rjk->rsik", ops, R).reshape(-1, 9)            # S^T R: trace((S G)^T R) = sum(G * S^T R)
    tr = (A @ G.reshape(-1, 9).T).reshape(len(R), -1).max(axis=1)
    return np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0)))


def test_restricted_grid_covers_the_rotations_modulo_the_group(grids):
    """The candidates of a symmetric reference are G N0 with G from the asymmetric unit, and pose N is as good as S N: every rotation
    must have an S G nearby.  400 random rotations: the largest distance at most 1.2 x the full grid's on the same sample, the mean at
    most 1.1 x (measured when the grid was designed: 1.16 and 1.07 at worst, C7 and D7 at 30 degrees)."""
    from oracle import oracle as O
    R = random_rotations(400, 20240917)
    for step in STEPS:
        full = nearest_deg(R, np.eye(3)[None], grids[(step, "")])
        for sym in SYMBOLS:
            d = nearest_deg(R, O.symmetry_ops(sym), grids[(step, sym)])
            print("step %g %-3s grid %4d: max %.2f deg (%.3f x C1's %.2f), mean %.2f (%.3f x)" % (
                step, sym, len(grids[(step, sym)]), d.max(), d.max() / full.max(), full.max(), d.mean(), d.mean() / full.mean()))
            assert d.max() <= 1.2 * full.max() and d.mean() <= 1.1 * full.mean(), (step, sym)


def test_svacfg_mirror_has_the_size_of_the_c_struct(tmp_path):
    (tmp_path / "s.cpp").write_text(SIZE_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(tmp_path / "s.cpp")])
    assert ctypes.sizeof(SvaCfg) == int(subprocess.check_output([str(tmp_path / "s")]).decode())
    assert SvaCfg._fields_[-1][0] == "symmetry" and SvaCfg.symmetry.offset + 8 == ctypes.sizeof(SvaCfg)
    assert SvaCfg.make(32).symmetry == b"" and SvaCfg.make(32, symmetry="D7").symmetry == b"D7"


PROTOCOL = """<config><general><mode>3</mode><metric><use_missing_wedge>1</use_missing_wedge></metric></general>
  <mra><mra_image_window_x>12</mra_image_window_x><mra_low_pass_cutoff>0.30</mra_low_pass_cutoff>%s</mra></config>"""


def test_protocol_symmetry_order_is_read_or_refused(tmp_path):
    from pyp_amd import sva
    xml = tmp_path / "iteration_006_mode_3.xml"

    def cfg(field):
        xml.write_text(PROTOCOL % ("" if field is None else "<mra_use_symmetrization>%s</mra_use_symmetrization>" % field))
        return sva.cfg_from_xml(str(xml), 32)
    assert cfg("3").symmetry == b"C3" and sva.symmetry_of(cfg("3")) == "C3"
    assert cfg("60").symmetry == b"C60"
    for none in ("1", "0", None):
        assert cfg(none).symmetry == b"" and sva.symmetry_of(cfg(none)) == "C1"
    for bad in ("-2", "61", "x"):
        with pytest.raises(ValueError, match="ERROR"):
            cfg(bad)
