"""The recomputed map normals (csrc/normals.hip: get_normals = 0, count mode) at their edges, through a
census that makes every map normal observable in ImlsContext.project — map_normals_cases.py builds the
cases and the census, test_map_normals_cases.py proves on the CPU that each case reaches its edge and
that its census is complete.

For every map state reached, census() asserts:
  1. device against oracle: x, n, idx and the reject counters bit-equal to oracle_ctypes.project, y within
     1e-5 (the projection's parity contract);
  2. device against map_normals_np (brute-force lists, LAPACK eigh): n[row] within one float32 ulp at 1.0
     (2⁻²³) of float32(restated normal of point idx[row]) where the eigenvalue gap is healthy; elsewhere
     (K = 1, K = 2) ‖C·n‖ within map_normals_np.residual's bound;
  3. reject[invalid_normal] = the restated number of ∞ normals;
  4. the valid rows cover ≥ 95 % of the finite-normal points.
Contexts are module-level; references and oracle results are cached per (map, K, r).

Measured on an MI355X over the file's 68 censuses (67,250 rows): device n against the restatement 0 (the
same float on every row), y against the oracle ≤ 2.4e-7.  test_failed_batch_leaves_no_normals_claimed
failed before frames_async set the validity flag after its launch (153 of 700 rows rejected by the angle
gate against the previous map's normals)."""
import numpy as np
import pytest

import gpu_mem
import map_normals_cases as mc
import map_normals_np as mn
import model_restatement as mr
import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, imls_icp

pytestmark = pytest.mark.gpu
TRAVERSALS = {"auto": _abi.IMLS_TRAVERSAL_AUTO, "packets": _abi.IMLS_TRAVERSAL_PACKETS, "lane": _abi.IMLS_TRAVERSAL_LANE}
Y_TOL = 1e-5                 # the projection's parity contract
POSE_TOL = 1e-6

_CTX = {}


def ctx_for(leaf=64, tag=""):
    key = (leaf, tag)
    if key not in _CTX:
        c = imls_icp.ImlsContext(mc.params(10, 1.0))
        c.set_option("leaf_size", leaf)
        _CTX[key] = c
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def soa(rows):
    return np.ascontiguousarray(np.asarray(rows, np.float32).T)


def census(c, P, K, r, gate=True, healthy=True, label="", set_params=True):
    """Assertions 1 – 4 on context c, whose target is map P."""
    ref = mc.reference(P, K, r)
    wx, wy, wn, widx, wrej = mc.oracle_census(P, K, r, gate)
    if set_params:
        c.set_params(mc.params(K, r, gate))
    kept = c.set_source(ref.src)
    assert len(kept) == len(ref.P), label
    x, y, n, idx, rej = c.project()
    assert np.array_equal(rej, wrej), (label, rej, wrej)
    assert np.array_equal(idx, widx), label
    bad = np.nonzero((n != wn).any(axis=1))[0]
    assert bad.size == 0, (label, len(bad), idx[bad[:3]], n[bad[:3]], wn[bad[:3]])
    assert np.array_equal(x, wx) and np.array_equal(n, wn), label
    dy = float(np.abs(y.astype(np.float64) - wy).max()) if len(idx) else 0.0
    err = mc.check_against_restatement(ref, n, idx, rej, healthy, label)
    print(f"census {label}: M {len(ref.P)} valid {len(idx)} ∞ {ref.n_inf} |n − restatement| {err:.3e} |y − oracle| {dy:.3e}")
    assert dy <= Y_TOL, (label, dy)


def load(c, P):
    assert c.set_target(mc.map_rows(P)) == len(P)


# ---- every case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,leaf", [(n, 64) for n in mc.CASES] + [(n, 4) for n in mc.LEAF_CASES])
def test_census(name, leaf):
    case = mc.CASES[name]
    c = ctx_for(leaf)
    load(c, case.points())
    census(c, case.points(), case.K, case.r, case.gate, case.healthy, f"{name}/leaf{leaf}")


@pytest.mark.parametrize("trav", ["packets", "lane"])
@pytest.mark.parametrize("name", mc.TRAVERSAL_CASES + ("duplicates-K12",))
def test_census_read_by_every_traversal(name, trav):
    """The projection kernels of the packet and the per-lane traversal read the normals too (auto is
    test_census); duplicates-K12 has 4,500 queries: the large-frame kernels."""
    case = mc.CASES[name]
    c = ctx_for(64, "traversal")
    try:
        c.set_option("traversal", TRAVERSALS[trav])
        load(c, case.points())
        census(c, case.points(), case.K, case.r, case.gate, case.healthy, f"{name}/{trav}")
    finally:
        c.set_option("traversal", _abi.IMLS_TRAVERSAL_AUTO)


def _refused(c, K):
    with pytest.raises(_abi.ImlsError) as e:
        c.set_params(mc.params(K, 1.0))
    return e.value.status


def test_k_out_of_range_is_refused_and_the_context_goes_on():
    """search_number_normal = 0 and 33 (no rung holds them) are refused by set_params with IMLS_ERR_ARG
    (api.hip check_params); the params in force stay, and the context computes the next census as if
    nothing had happened."""
    case = mc.CASES["rung-K9"]
    c = ctx_for(64, "refused")
    load(c, case.points())
    census(c, case.points(), case.K, case.r, label="before the refusals")
    for K in (0, 33):
        assert _refused(c, K) == _abi.IMLS_ERR_ARG
        assert c.params.search_number_normal == case.K
        census(c, case.points(), case.K, case.r, label=f"after K = {K} was refused", set_params=False)
    census(c, case.points(), 17, case.r, label="K = 17 after the refusals")


# ---- map kinds and the validity flag ----------------------------------------------------------------------------------
def test_every_map_change_recomputes_the_normals():
    """One context in count mode; after every way of changing its map the census must give the normals of
    the map as it then is (consecutive maps share no normal: test_map_normals_cases.py).  The expected
    maps come from model_restatement.pose_cloud and voxel_map_np.update; the voxel map is also downloaded."""
    g, maps = mc.kind_inputs(), dict(mc.kind_maps())
    K, r = mc.KIND_K, mc.KIND_R
    p = mc.params(K, r)
    p.max_queue_size = mc.KIND_QUEUE

    def check(stage, n=None):
        if n is not None:
            assert n == len(maps[stage]), stage
        census(c, maps[stage], K, r, label=f"kind/{stage}", set_params=False)

    with imls_icp.ImlsContext(p) as c:
        check("host", c.set_target(g["host"]))
        dev = gpu_mem.DevSoa(soa(g["device"]))
        try:
            c.set_defer(True)                       # the buffer is read at the first use: the census
            c.set_target_device(dev.ptr, len(g["device"]), count=False)
            check("device")
            c.set_defer(False)
            c.synchronize()
        finally:
            dev.free()
        for run in g["runs"]:                       # three runs of the lattice: ties cross them
            n = c.map_push(run)
        check("fifo", n)
        c.map_clear()
        check("posed", c.map_push(g["posed_scan"], pose=g["posed_pose"]))
        c.map_rebase(g["rebase_pose"])
        check("rebased")
        c.map_clear()
        c.set_voxel_map_params(**mc.KIND_VOXEL)
        for k in (1, 2):
            n = c.voxel_map_update(g[f"voxel_scan{k}"], g[f"voxel_pose{k}"])
            assert np.array_equal(c.voxel_map_download()[:3].T, maps[f"voxel{k}"])
            check(f"voxel{k}", n)
        c.map_clear()
        check("cleared", c.map_push(mc.map_rows(maps["cleared"])))


# ---- parameters --------------------------------------------------------------------------------------------------
def test_parameters_back_and_forth():
    """A fixed map: (K, r) changed and changed back (the flag is valid, its K or r is not), then
    get_normals 1 → 0 → 1 → 0 with stored normals (0.6, 0, 0.8) no recomputed normal equals."""
    P = mc.plane()
    c = ctx_for(64, "params")
    load(c, P)
    for K, r in ((8, 1.0), (9, 1.0), (8, 1.0), (10, 0.3), (8, 1.0), (10, 1.0), (10, 0.3)):
        census(c, P, K, r, label=f"params/K{K}-r{r}")
    ref = mc.reference(P, 9, 1.0)
    for get_normals in (1, 0, 1, 0):
        if not get_normals:
            census(c, P, 9, 1.0, gate=False, label="params/get_normals 0")
            continue
        c.set_params(mc.params(9, 1.0, False, get_normals=1))
        c.set_source(ref.src)
        x, y, n, idx, rej = c.project()
        wx, wy, wn, widx, wrej = mc.oracle_census(P, 9, 1.0, False, get_normals=1)
        assert np.array_equal(rej, wrej) and np.array_equal(idx, widx) and np.array_equal(x, wx) and np.array_equal(n, wn)
        assert len(idx) == len(P) and np.array_equal(n, np.broadcast_to(np.float32(mc.STORED), n.shape))
        assert np.abs(y.astype(np.float64) - wy).max() <= Y_TOL


# ---- batches -----------------------------------------------------------------------------------------------------
def _frame(c, P, tensors=False):
    load(c, P)
    if tensors:
        c.set_target_tensors(mc.plate_tensors(P))
    c.set_source(mc.registration_source(P))


def _alone(P, p, tensors=False):
    with imls_icp.ImlsContext(p) as c:
        _frame(c, P, tensors)
        return c.register_frame()


def test_fused_batch_computes_every_members_normals():
    """register_frames over three contexts with LS and the packet traversal — fused (api_frames.hip
    batch_fusable: no per-lane mode, no projected distance, an LS-family solver; n ≥ 2), so the normals of
    the members that lack them come from ONE k_map_normals_b launch: maps of 1,500, 700 and 100 points
    (grid x sized by the largest, the smallest below one block), and one member whose normals are already
    valid from an earlier project (its recompute_normals flag is 0: the kernel must leave it alone)."""
    maps = mc.batch_maps()
    K, r = mc.BATCH_K, mc.BATCH_R
    p = mc.params(K, r, iters=mc.BATCH_ITERS)
    ctxs = [imls_icp.ImlsContext(p) for _ in maps]
    try:
        load(ctxs[1], maps[1])
        census(ctxs[1], maps[1], K, r, label="batch/member 1 before", set_params=False)
        _frame(ctxs[0], maps[0])
        ctxs[1].set_source(mc.registration_source(maps[1]))         # (a set_target would drop its normals)
        _frame(ctxs[2], maps[2])
        poses, iters, status, _ = imls_icp.register_frames(ctxs)
        for k, P in enumerate(maps):
            one = _alone(P, p)
            assert np.array_equal(one["pose"], poses[k]) and (one["iters"], one["status"]) == (iters[k], status[k]), k
            want = oc.register_frame(soa(mc.registration_source(P)), soa(mc.map_rows(P)), p)
            assert (want["iters"], want["status"]) == (iters[k], status[k]) and iters[k] == mc.BATCH_ITERS, k
            assert np.abs(poses[k] - want["pose"]).max() < POSE_TOL, k
        for k, (c, P) in enumerate(zip(ctxs, maps)):
            # api.hip ensure_map_normals returns at once while the flag is set with this K and r: the
            # normals this census reads are the ones k_map_normals_b wrote (member 1: k_map_normals)
            census(c, P, K, r, label=f"batch/member {k} after", set_params=False)
    finally:
        for c in ctxs:
            c.close()


def test_failed_batch_leaves_no_normals_claimed():
    """A batch that fails a member's check after flagging an earlier member's normals as computed
    (api_frames.hip frames_async: tensor voting on, member B without tensors → IMLS_ERR_STATE) has
    launched nothing: member A's next project must compute the normals of its current map, not read
    the previous map's from its buffer."""
    old, new, other = mc.failed_batch_maps()
    K, r = mc.BATCH_K, mc.BATCH_R
    p_tv = mc.params(K, r, iters=mc.BATCH_ITERS, tensor_voting=1)
    with imls_icp.ImlsContext(p_tv) as A, imls_icp.ImlsContext(p_tv) as B:
        _frame(A, old, tensors=True)
        assert A.register_frame()["iters"] == mc.BATCH_ITERS     # A's buffer now holds the old map's normals
        _frame(A, new, tensors=True)
        _frame(B, other)                                          # no tensors
        with pytest.raises(_abi.ImlsError) as e:
            imls_icp.register_frames([A, B])
        assert e.value.status == _abi.IMLS_ERR_STATE
        B.set_target_tensors(mc.plate_tensors(other))
        census(A, new, K, r, label="failed batch/A")              # count mode without tensor voting, same K and r
        A.set_params(p_tv)
        A.set_source(mc.registration_source(new))
        poses, iters, status, _ = imls_icp.register_frames([A, B])
    for k, P in enumerate((new, other)):
        one = _alone(P, p_tv, tensors=True)
        assert np.array_equal(one["pose"], poses[k]) and (one["iters"], one["status"]) == (iters[k], status[k]), k
        assert iters[k] == mc.BATCH_ITERS
