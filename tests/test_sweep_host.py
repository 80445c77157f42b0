"""CPU tests of the sweep-to-pose entry points (imls_sweep_process and what rides on it): the C
structs against their ctypes mirrors, the defaults, the host-drawn shuffles as positions against the
oracle's shuffle, and the Python entry points that must fail or validate without a GPU."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, imls_icp, producer

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "imls_gpu.h"


def _walk(ctype, prefix=""):
    """Every leaf field of a (nested) ctypes structure as (C member designator, offset)."""
    for name, t in ctype._fields_:
        off = getattr(ctype, name).offset
        if issubclass(t, C.Structure):
            yield prefix + name, off
            for sub, o in _walk(t, prefix + name + "."):
                yield sub, off + o
        else:
            yield prefix + name, off


@pytest.mark.parametrize("ctype,cname", [(_abi.ImlsSweepParams, "imls_sweep_params"),
                                          (_abi.ImlsSweepInfo, "imls_sweep_info")])
def test_sweep_struct_layouts_match_c(tmp_path, ctype, cname):
    members = list(_walk(ctype))
    prog = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){",
            f'printf("%zu\\n", sizeof({cname}));']
    prog += [f'printf("%zu\\n", offsetof({cname}, {m}));' for m, _ in members]
    prog += ["return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == C.sizeof(ctype)
    assert len(members) >= 13
    for (m, off), c_off in zip(members, vals[1:]):
        assert off == c_off, m


def _leaves(p, prefix=""):
    out = {}
    for name, t in p._fields_:
        v = getattr(p, name)
        if issubclass(t, C.Structure):
            out.update(_leaves(v, prefix + name + "."))
        else:
            out[prefix + name] = v
    return out


def test_default_sweep_params_equal_the_defaults_of_the_parts():
    lib = _abi.load_library()
    p = _abi.ImlsSweepParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    lib.imls_default_sweep_params(C.byref(p))
    front, pca, curv = _abi.ImlsFrontParams(), _abi.ImlsPcaParams(), _abi.ImlsCurvatureParams()
    nrm, maj = _abi.ImlsSampleParams(), _abi.ImlsSampleParams()
    lib.imls_default_front_params(C.byref(front))
    lib.imls_default_pca_params(C.byref(pca))
    lib.imls_default_curvature_params(C.byref(curv))
    lib.imls_default_sample_params(C.byref(nrm), _abi.IMLS_SAMPLE_NORMAL)
    lib.imls_default_sample_params(C.byref(maj), _abi.IMLS_SAMPLE_MAJOR_AXIS)
    for got, want in ((p.front, front), (p.pca, pca), (p.curvature, curv), (p.normal, nrm), (p.major_axis, maj)):
        assert _leaves(got) == _leaves(want)
    # the shipped chain: pca → geometric_features → major_axis
    assert (p.presample_method, p.sample_method) == (_abi.IMLS_PRESAMPLE_GEOMETRIC_FEATURES, _abi.IMLS_SWEEP_MAJOR_AXIS)
    assert (p.points_per_list, p.max_points, p.shuffle_seed, p.rand_seed) == (200, 2000, 0, 1)
    assert _leaves(p) == _leaves(_abi.default_sweep_params())


def _positions(seed, size, k):
    out = np.zeros(max(min(k, size), 1), np.int32)
    n = C.c_size_t()
    _abi.load_library().imls_shuffle_positions(seed, size, k, out.ctypes.data_as(C.c_void_p), C.byref(n))
    return out[:n.value]


def _oracle_shuffle(bin_, k, seed):
    """randomSampling(bin, k) through the oracle: normalSampling on one bin, min_points 0, random
    strategy — one call with the seed's generator (needs len(bin) > k)."""
    n = int(bin_.max()) + 1
    xyz = np.zeros((n, 3), np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n, 1))
    p = _abi.default_sample_params(_abi.IMLS_SAMPLE_NORMAL)
    p.azimuth_bins = p.elevation_bins = 1
    p.min_points_per_bin, p.max_points_per_bin = 0, k
    p.sampling_strategy, p.shuffle_seed = _abi.SAMPLE_RANDOM, seed
    return oc.sample_point_cloud(xyz, nrm, bin_, None, p)[0]


@pytest.mark.parametrize("size", [1, 2, 3, 201, 5000])
def test_shuffled_positions_index_the_shuffled_bin(size):
    """Shuffling 0 … size−1 and indexing the bin equals shuffling the bin (the oracle's shuffle)."""
    rng = np.random.default_rng(size)
    bin_ = rng.permutation(7 * size + 11)[:size].astype(np.int32)       # distinct, unordered contents
    for seed in (0, 7919 * 3 + 5):
        pos = _positions(seed, size, size)                               # the whole permutation
        assert sorted(pos.tolist()) == list(range(size))
        for k in sorted({size - 1, min(200, size - 1), size // 2}):
            want = _oracle_shuffle(bin_, k, seed)
            assert len(want) == k
            assert np.array_equal(bin_[_positions(seed, size, k)], want)
            assert np.array_equal(pos[:k], _positions(seed, size, k))    # a prefix of the permutation
    assert len(_positions(3, size, 0)) == 0 and len(_positions(3, size, -5)) == 0
    assert len(_positions(3, size, size + 9)) == size


def test_process_sweep_without_a_producer_raises():
    lo = imls_icp.LaserOdometry.__new__(imls_icp.LaserOdometry)    # no context: the check comes before any GPU use
    lo.producer = None
    with pytest.raises(ValueError, match="producer"):
        lo.process_sweep(np.zeros((4, 3), np.float32))


def test_producer_from_config_builds_sweep_params_without_a_gpu():
    cfg = config.load()
    sr = config.producer_from_config(cfg, shuffle_seed=11, rand_seed=5)
    assert isinstance(sr, producer.ScanRegistration) and sr._ctx is None
    sp = sr.sweep_params()
    assert sr._ctx is None                                            # still lazy
    want = _abi.default_sweep_params()
    want.shuffle_seed, want.rand_seed = (11 + 7919) & 0xFFFFFFFF, 5
    assert _leaves(sp) == _leaves(want)
    sr.frame = 4
    sp = sr.sweep_params(_abi.ImlsFrontParams(16, 1.0, 90.0, 0.1, 1))
    assert (sp.shuffle_seed, sp.rand_seed) == ((11 + 7919 * 4) & 0xFFFFFFFF, 8)
    assert (sp.front.n_scans, sp.front.minimum_range, sp.front.is_dense) == (16, 1.0, 1)
    sr = producer.ScanRegistration(sample_method="three_axis", presample_method="curvature", points_per_list=64,
                                   max_points=500)
    sp = sr.sweep_params()
    assert (sp.presample_method, sp.sample_method, sp.points_per_list, sp.max_points) == (
        _abi.IMLS_PRESAMPLE_CURVATURE, _abi.IMLS_SWEEP_THREE_AXIS, 64, 500)
