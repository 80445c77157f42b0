"""Debug-trace build (IMLS_LIB_PATH=…/debug/libimls_gpu.so): the per-wave records of the packet
traversal, saved so that two builds can be compared wave for wave ("same work": same leaves, inner
nodes, sparse and broadcast visits, wanting-lane trips, insertion steps and insertions).

    IMLS_LIB_PATH=<debug build> python tools/wave_records.py dump OUT.npz
    python tools/wave_records.py compare A.npz B.npz

dump records, at 64-query packets: each of a config-B pair's 20 launches; the inputs of
tests/test_gpu_knn_steps.py (projections at leaf 64 / 16 / 4, the registration's 6 launches); the
inputs of tests/test_gpu_knn_scalar_paths.py.  compare checks every column but the two clock columns;
column 12 carries the visits with a listed point in its low half and, from round 8 on, the sparse
visits that built the listed mask in its high half (printed, not compared).
"""
import ctypes as C, pathlib, sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
COLS = ["seed_t", "trav_t", "leaves", "inner", "ins_steps", "sparse_lv", "bcast_lv", "greedy", "W_inf", "W>1", "Wmax",
        "sp_trips", "sp_listed_lv", "ins", "seed_steps", "seed_pts"]


def dump(out):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "oracle"))
    sys.path.insert(0, str(ROOT / "tests"))
    import plo_amd
    plo_amd.load()
    from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth
    import test_gpu_knn_steps as steps
    import test_gpu_knn_scalar_paths as paths

    rec = {}

    def run(name, tgt, src, iters, leaf=None, project=False, K=None):
        p = config.bench_params(iters)
        if K:
            p.search_number = K
        c = imls_icp.ImlsContext(p, device=0)
        c.set_option("traversal", _abi.IMLS_TRAVERSAL_PACKETS)
        c.set_option("first_packet", 64)
        if leaf:
            c.set_option("leaf_size", leaf)
        c.set_target(tgt)
        c.set_source(src)
        c.project(np.eye(4)) if project else c.register_frame()
        buf = np.zeros((8192, 16), np.uint32)
        c.lib.imls_debug_waves(C.c_void_p(buf.ctypes.data), 8192)
        c.close()
        rec[name] = buf[:min(8192, (src.size + 63) // 64)].copy()

    pair = synth.make_pairs(1, "hdl64", map_scans=10, scene_seed=0, traj_seed=2000, noise_seed=1000)[0]
    for it in range(1, 21):
        run(f"B_launch{it - 1:02d}", pair.target, pair.source, it)
    cl = steps.build_clouds()
    for leaf in (64, 16, 4):
        for name in ("spread", "clustered"):
            run(f"steps_{name}_leaf{leaf}", cl["tgt"], cl[name], steps.ITERS, leaf=leaf, project=True)
    for it in range(1, steps.ITERS + 1):
        run(f"steps_reg_launch{it - 1}", cl["tgt"], cl["reg"], it)
    pc = paths.build_clouds()
    for n, src in pc["lone"].items():
        run(f"paths_lone{n}", pc["tgt"], src, paths.ITERS, project=True)
    for m, tgt in pc["small"].items():
        run(f"paths_small{m}", tgt, pc["small_src"][m], paths.ITERS, leaf=64, project=True, K=8)
    for leaf in (64, 16):
        for it in range(1, paths.ITERS + 1):
            run(f"paths_half_leaf{leaf}_launch{it - 1}", pc["tgt"], pc["half"], it, leaf=leaf)
    run("paths_tie", pc["tgt"], pc["tie"], paths.ITERS, project=True)
    np.savez_compressed(out, **rec)
    print(f"{len(rec)} launches recorded in {out}")


def compare(fa, fb):
    a, b = np.load(fa), np.load(fb)
    assert sorted(a.files) == sorted(b.files), "different launches recorded"
    bad = 0
    tot = {}
    for k in sorted(a.files):
        x, y = a[k].copy(), b[k].copy()
        mx, my = x[:, 12] >> 16, y[:, 12] >> 16
        x[:, 12] &= 0xFFFF
        y[:, 12] &= 0xFFFF
        same = np.array_equal(x[:, 2:], y[:, 2:])
        bad += 0 if same else 1
        s = y.astype(np.int64).sum(0)
        grp = k.split("_launch")[0]
        t = tot.setdefault(grp, np.zeros(7, np.int64))
        t += (len(y), s[5], s[6], s[11], s[4], int(my.sum()), s[3])
        print(f"{k:32s} waves {len(x):5d} {'identical' if same else 'DIFFERENT'}  sparse {s[5]:7d} bcast {s[6]:6d} "
              f"trips {s[11]:8d} ins_steps {s[4]:8d} ins {s[13]:8d} inner {s[3]:7d} leaves {s[2]:7d} "
              f"listed_lv {s[12]:7d} mask_built {int(mx.sum())} / {int(my.sum())}")
    for g, t in tot.items():
        print(f"total {g:28s} wave-launches {t[0]} sparse {t[1]} bcast {t[2]} trips {t[3]} ins_steps {t[4]} mask_built(B) {t[5]} inner {t[6]}")
    print("ALL IDENTICAL" if bad == 0 else f"{bad} launches differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
