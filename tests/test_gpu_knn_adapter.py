"""GPU: the C++ adapter's libnabo-shaped kNN.  A small program written here includes
include/imls_icp_hip.hpp, loads a target and queries from raw float files, calls
imls_hip::NNSearchHip::knn with a libnabo call site's argument list (imls_icp.cpp:605-607) and dumps
the indices and d²; it is compiled with the host g++ against the in-tree libimls_gpu.so (rpath) and
run as a child process.  Its rows must equal ImlsContext.knn and the oracle, exactly; epsilon != 0
takes the adapter's error path (IMLS_ERR_UNSUPPORTED)."""
import pathlib
import subprocess

import numpy as np
import pytest

import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, imls_icp

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
LIBDIR = ROOT / "planetary-lidar-odometry_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden"

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "imls_icp_hip.hpp"
static std::vector<float> load(const char* path) {
    std::vector<float> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(3);
    float b[4096];
    size_t n;
    while ((n = std::fread(b, 4, 4096, f)) > 0) v.insert(v.end(), b, b + n);
    std::fclose(f);
    return v;
}
int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const std::vector<float> tgt = load(argv[1]);           // rows x y z nx ny nz
    const std::vector<float> qf = load(argv[2]);            // rows x y z
    const int K = std::atoi(argv[3]);
    const double r = std::atof(argv[4]), eps = std::atof(argv[5]);
    const unsigned flags = (unsigned)std::atoi(argv[6]);
    const size_t M = tgt.size() / 6, Q = qf.size() / 3;
    try {
        imls_hip::IMLSICPMatcherHip matcher;
        imls_hip::detail::check(imls_set_target(matcher.context(), tgt.data(), tgt.data() + 3, M, 6, nullptr), matcher.context());
        imls_hip::NNSearchHip tree(matcher);
        std::vector<double> query(qf.begin(), qf.end());    // 3 x Q column-major doubles
        std::vector<int> indices(K * Q);
        std::vector<double> dists2(K * Q);
        const unsigned long total = tree.knn(query.data(), Q, indices.data(), dists2.data(), K, eps, flags, r);
        FILE* f = std::fopen(argv[7], "wb");
        std::fwrite(indices.data(), sizeof(int), indices.size(), f);
        std::fwrite(dists2.data(), sizeof(double), dists2.size(), f);
        std::fclose(f);
        std::printf("total %lu\n", total);
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 1;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("knn_adapter")
    src = d / "knn_adapter.cpp"
    src.write_text(PROGRAM)
    out = d / "knn_adapter"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", f"-I{ROOT / 'include'}", "-o", str(out), str(src),
                    f"-L{LIBDIR}", "-limls_gpu", f"-Wl,-rpath,{LIBDIR}"], check=True)
    return out


def run(exe, tmp_path, tgt6, q, k, r, eps, flags):
    np.ascontiguousarray(tgt6.T, np.float32).tofile(tmp_path / "tgt.bin")
    np.ascontiguousarray(q, np.float32).tofile(tmp_path / "q.bin")
    out = tmp_path / "out.bin"
    p = subprocess.run([str(exe), str(tmp_path / "tgt.bin"), str(tmp_path / "q.bin"), str(k), repr(float(r)), repr(eps),
                        str(flags), str(out)], capture_output=True, text=True, timeout=120)
    return p, out


@pytest.mark.parametrize("flags,self_ok", [(2, False), (2 | 1 | 4, True)])   # SORT_RESULTS [| ALLOW_SELF_MATCH | TOUCH_STATISTICS]
def test_adapter_knn_equals_context_and_oracle(exe, tmp_path, flags, self_ok):
    g = np.load(GOLDEN / "planetary_pair.npz")
    tgt = np.ascontiguousarray(g["tgt"], np.float32)
    q = np.ascontiguousarray(g["tgt"][:3, ::9].T, np.float32)          # map points: self matches matter
    k, r = 10, 1.0
    p, out = run(exe, tmp_path, tgt, q, k, r, 0.0, flags)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = out.read_bytes()
    idx = np.frombuffer(raw[: len(q) * k * 4], np.int32).reshape(len(q), k)
    d2 = np.frombuffer(raw[len(q) * k * 4:], np.float64).reshape(len(q), k)
    wd2, widx = oc.knn(tgt, np.ascontiguousarray(q.T), k, r, self_ok)
    assert np.array_equal(idx, widx) and np.array_equal(d2, wd2)
    assert int(p.stdout.split()[1]) == int((widx >= 0).sum())
    with imls_icp.ImlsContext(config.bench_params(3)) as c:
        c.set_target(np.ascontiguousarray(tgt.T))
        cidx, cd2, found = c.knn(q, k, r, self_ok)
    assert np.array_equal(idx, cidx) and np.array_equal(d2, cd2)


def test_adapter_rejects_epsilon(exe, tmp_path):
    g = np.load(GOLDEN / "planetary_pair.npz")
    tgt = np.ascontiguousarray(g["tgt"], np.float32)
    p, _ = run(exe, tmp_path, tgt, tgt[:3, :20].T, 4, 1.0, 0.1, 2)
    assert p.returncode == 1 and f"status {_abi.IMLS_ERR_UNSUPPORTED}" in p.stdout, p.stdout + p.stderr
