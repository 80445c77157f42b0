"""Debug-trace build: per-launch leaf-visit counts of a config-B pair over all 20 ICP iterations (64-query
packets, as the batched launches use), and the scan paths the new tests' inputs reach."""
import ctypes as C, pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import plo_amd
plo_amd.load()
import numpy as np
from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth


def waves(c, n):
    buf = np.zeros((8192, 16), np.uint32)
    c.lib.imls_debug_waves(C.c_void_p(buf.ctypes.data), 8192)
    return buf[:n].astype(np.float64)


pair = synth.make_pairs(1, "hdl64", map_scans=10, scene_seed=0, traj_seed=2000, noise_seed=1000)[0]
N = pair.source.size
nw = (N + 63) // 64
print(f"config B pair: {N} queries, {nw} waves of 64")
tot = np.zeros(4)
for iters in range(1, 21):
    c = imls_icp.ImlsContext(config.bench_params(iters), device=0)
    c.set_option("traversal", _abi.IMLS_TRAVERSAL_PACKETS)
    c.set_option("first_packet", 64)
    c.set_target(pair.target)
    c.set_source(pair.source)
    c.register_frame()
    a = waves(c, nw)
    sp, bc, lst, lv = a[:, 5].mean(), a[:, 6].mean(), a[:, 12].mean(), a[:, 2].mean()
    tot += (sp, bc, lst, 49 * sp + 72 * bc)
    print(f"launch {iters - 1:2d}: leaves {lv:6.2f} sparse {sp:6.2f} bcast {bc:5.2f} sparse-with-listed {lst:6.2f} "
          f"share {lst / max(sp, 1e-9):.3f}  49*sparse+72*bcast {49 * sp + 72 * bc:7.1f}")
    c.close()
tot /= 20
print(f"mean over 20 launches per wave: sparse {tot[0]:.2f} bcast {tot[1]:.2f} sparse-with-listed {tot[2]:.2f} "
      f"(share {tot[2] / tot[0]:.3f}); copies removed statically 49*sparse+72*bcast = {tot[3]:.0f} VALU per wave")

# the inputs of tests/test_gpu_knn_steps.py, from its own builder
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
from test_gpu_knn_steps import SRC_N, build_clouds
cl = build_clouds()
tgt = cl["tgt"]
for leaf in (64, 16, 4):
    for name in ("spread", "clustered"):
        src = cl[name]
        c = imls_icp.ImlsContext(config.bench_params(6), device=0)
        c.set_option("traversal", _abi.IMLS_TRAVERSAL_PACKETS)
        c.set_option("leaf_size", leaf)
        c.set_option("first_packet", 64)
        c.set_target(tgt)
        c.set_source(src)
        c.project(np.eye(4))
        a = waves(c, (SRC_N + 63) // 64)   # project(): 64-query packets
        print(f"test input leaf {leaf:2d} {name:9s}: sparse leaf visits {int(a[:, 5].sum())}, broadcast leaf visits {int(a[:, 6].sum())}")
        c.close()
