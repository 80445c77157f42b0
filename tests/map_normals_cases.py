"""Edge cases of the recomputed map normals (csrc/normals.hip: get_normals = 0, count mode), shared by
test_map_normals_cases.py — which proves on numpy and the CPU oracle alone that every case reaches the
edge it is named for — and test_gpu_map_normals.py, which runs them on the device.  No GPU imports.

normals.hip has a kNN of its own (one lane per map point, a capacity-K list inside KC ∈ {8, 16, 32}
registers with sentinels in the unused slots, fp32 box pruning with slack, (d², index) order, the self
match left out by d² > DBL_EPSILON), then the moments in list order, a 3×3 Jacobi and the flip to +z.
The matcher reads the result like stored normals.  Two references:

  map_normals_np   brute-force neighbour lists, fp64 moments in list order, np.linalg.eigh;
  the CPU oracle   oracle_ctypes.project (its own kd-tree, the Jacobi sweeps the device shares).

The census makes every map normal observable through the projection.  The projection's NN-1 search leaves
the self match out, so the query of map point i is float32(p_i + δ·n_i) with δ = 2⁻⁹ m — a power of two,
δ² = 3.8e-6 > DBL_EPSILON, far under every point spacing used here (0.02 m and more) — applied to the
float coordinates, at the identity pose, with n_i (map_normals_np's, rounded to float; (0, 0, 1) where it
is ∞) as the query's own normal.  Its NN-1 is point i (of exact copies: the lowest index among them), so
a valid row returns the recomputed normal of point i and a row whose point has an ∞ normal is counted in
reject[invalid_normal].  The census is complete when the valid rows cover ≥ 95 % of the finite-normal
points: a condition of every case, proved from the oracle alone.

Where the two smallest eigenvalues are not separated (K = 1, K = 2; map_normals_np.GAP) and at K = 3
(three points: λ0 = 0 and the normals of neighbouring triples scatter) the case turns the 30° angle gate
off (normal_angle_constraint = 0): the IMLS neighbours would otherwise be rejected for normals that are
arbitrary by construction, and the census would see 90 % of the points at K = 3.

Generators are seeded and deterministic; maps are (M, 3) float32 in map order.
"""
import functools
from dataclasses import dataclass

import numpy as np

import imls_np
import map_normals_np as mn

DELTA = 2.0 ** -9
COVERAGE = 0.95
STORED = (0.6, 0.0, 0.8)            # the stored normal of every map row: never a recomputed one here
REJ_INVALID = 2                     # _abi.REJECT_NAMES.index("invalid_normal")
REJ_MLS_FAIL = 4
KC_RUNGS = (8, 16, 32)              # normals.hip: the register capacities of launch_map_normals
NRM_BLOCK = 128                     # normals.hip kNrmBlock
LEAVES = (4, 64)
BIG_FRAME = 4096                    # internal.h kSmallRows: above it the large-frame kernels project


# ---- clouds ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane(M=1500, side=6.0, seed=1):
    """A noisy plane patch: M points uniform on side × side m, σ_z = 0.01."""
    rng = np.random.default_rng(seed)
    P = np.empty((M, 3))
    P[:, :2] = rng.uniform(0.0, side, (M, 2))
    P[:, 2] = rng.normal(0.0, 0.01, M)
    return np.ascontiguousarray(P.astype(np.float32))


@functools.lru_cache(maxsize=None)
def lattice(flat=False, shift=(0.0, 0.0, 0.0), n=24, seed=2):
    """n × n lattice, spacing 0.25, z = ((7i + 3j) mod 5) / 64 (flat: 0), rows shuffled: every coordinate
    is exact in float, with and without the shift, so equal distances are equal bit for bit."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    P = np.stack([0.25 * i, 0.25 * j, 0.0 * i if flat else ((7 * i + 3 * j) % 5) / 64.0], axis=-1).reshape(-1, 3)
    P = P[np.random.default_rng(seed).permutation(len(P))] + np.asarray(shift, np.float64)
    P32 = P.astype(np.float32)
    assert np.array_equal(P32.astype(np.float64), P)
    return np.ascontiguousarray(P32)


@functools.lru_cache(maxsize=None)
def duplicates(seed=3):
    """Every point of the plane patch stored three times, the copies spread over the map order."""
    P = np.concatenate([plane()] * 3)
    return np.ascontiguousarray(P[np.random.default_rng(seed).permutation(len(P))])


@functools.lru_cache(maxsize=None)
def cluster(M, seed=4):
    """M points of a compact, nearly flat cluster: 0.5 × 0.5 m, σ_z = 0.005 — every pair within r = 1."""
    rng = np.random.default_rng(seed + M)
    P = np.empty((M, 3))
    P[:, :2] = rng.uniform(0.0, 0.5, (M, 2))
    P[:, 2] = rng.normal(0.0, 0.005, M)
    return np.ascontiguousarray(P.astype(np.float32))


@functools.lru_cache(maxsize=None)
def islands(small=5, seed=5):
    """A 204-point patch (2 × 2 m) and `small` points 10 m away from it, in the middle of the map order
    (209 points: a multiple of neither leaf size)."""
    big = plane(204, 2.0, seed)
    far = cluster(small, seed) + np.float32([10.0, 10.0, 0.0])
    return np.ascontiguousarray(np.concatenate([big[:100], far, big[100:]]))


@functools.lru_cache(maxsize=None)
def pyramid(M, half=3.0, seed=6):
    """z = 0.4|x| + 0.3|y| + noise (σ 0.005) on [−half, half]²: four facets whose normals all point up
    and differ, so a registration against it is well conditioned in all six parameters."""
    rng = np.random.default_rng(seed + M)
    P = np.empty((M, 3))
    P[:, :2] = rng.uniform(-half, half, (M, 2))
    P[:, 2] = 0.4 * np.abs(P[:, 0]) + 0.3 * np.abs(P[:, 1]) + rng.normal(0.0, 0.005, M)
    return np.ascontiguousarray(P.astype(np.float32))


def map_rows(P, stored=STORED):
    """(M, 6) float32 map rows: the points with one stored normal (read only under get_normals = 1)."""
    P = np.asarray(P, np.float32).reshape(-1, 3)
    out = np.empty((len(P), 6), np.float32)
    out[:, :3] = P
    out[:, 3:] = np.float32(stored)
    return out


# ---- the cases ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    cloud: tuple                    # (generator name, args): points() builds the map
    K: int
    r: float
    gate: bool = True               # normal_angle_constraint of the census projection
    healthy: bool = True            # every finite row's relative eigenvalue gap ≥ mn.GAP
    n_inf: object = None            # the expected number of ∞ normals (None: not stated)

    def points(self):
        return globals()[self.cloud[0]](*self.cloud[1:])


R_BELOW = float(np.nextafter(0.25, 0.0))
PLANE, LAT, FLAT = ("plane",), ("lattice",), ("lattice", True)
LAT_SHIFTED = ("lattice", False, (1e5, -1e5, 512.0))
SIZES_K = 5                         # inside the first rung: three sentinel slots


def _cases():
    out = []
    # rungs: K = 1 and 2 (no gap), 3, and both sides of every KC edge: K = KC has no sentinel slot,
    # K = KC + 1 is the first of the next rung with KC − 1 of them
    for K in (1, 2, 3, 8, 9, 16, 17, 32):
        # (K = 32: one corner point of the patch has fewer than 32 points within 1 m)
        out.append(Case(f"rung-K{K}", PLANE, K, 1.0, gate=K > 3, healthy=K >= 3, n_inf=1 if K == 32 else 0))
    # the radius decides who has K neighbours
    out.append(Case("radius-plane-K10-r0.3", PLANE, 10, 0.3))
    # ties: equal d² everywhere, broken by the index
    for K in (6, 8, 13):
        out.append(Case(f"ties-K{K}", LAT, K, 1.0, n_inf=0))
    for K in (6, 13):
        out.append(Case(f"ties-shifted-K{K}", LAT_SHIFTED, K, 1.0, n_inf=0))
    # the radius edge: the four axis neighbours of the flat lattice sit at d² = r² exactly
    out.append(Case("radius-edge-K4", FLAT, 4, 0.25, n_inf=24 * 24 - 22 * 22))
    out.append(Case("radius-edge-K5", FLAT, 5, 0.25, n_inf=24 * 24))
    out.append(Case("radius-below-K4", FLAT, 4, R_BELOW, n_inf=24 * 24))
    # the whole map inside the ball: the boxes prune only once the list is full
    out.append(Case("radius-1e3-K13", LAT, 13, 1e3, n_inf=0))
    # duplicates (4,500 queries: above BIG_FRAME, the large-frame kernels read the normals too)
    out.append(Case("duplicates-K12", ("duplicates",), 12, 1.0, n_inf=0))
    # sizes: below, on and above K, the block (128) and both leaf sizes
    for M in (1, SIZES_K, SIZES_K + 1, 127, 128, 129):
        out.append(Case(f"size-M{M}", ("cluster", M), SIZES_K, 1.0, n_inf=M if M <= SIZES_K else 0))
    out.append(Case("islands", ("islands",), SIZES_K, 1.0))
    return {c.name: c for c in out}


CASES = _cases()
TRAVERSAL_CASES = ("rung-K9", "ties-K13", "radius-edge-K4")
LEAF_CASES = tuple(n for n in CASES if n.startswith("size-") or n == "islands") + ("ties-K6",)


# ---- references, computed once per (map, K, r) --------------------------------------------------------------
@dataclass(frozen=True)
class Ref:
    P: np.ndarray                   # (M, 3) float32 map
    K: int
    r: float
    nrm: np.ndarray                 # (M, 3) float64, ∞ rows where fewer than K neighbours
    lists: list
    lam: np.ndarray                 # (M, 3) eigenvalues ascending, NaN on the ∞ rows
    C: np.ndarray                   # (M, 3, 3) covariances
    finite: np.ndarray              # (M,) bool
    src: np.ndarray                 # (M, 6) float32 census queries

    @property
    def n_inf(self):
        return int((~self.finite).sum())

    @property
    def min_gap(self):
        return float(mn.rel_gap(self.lam)[self.finite].min()) if self.finite.any() else np.inf


_REF, _ORACLE = {}, {}


def census_queries(P, nrm, delta=DELTA):
    """(M, 6) float32: float32(p_i + δ·n_i) and n_i, (0, 0, 1) standing in for an ∞ normal."""
    P = np.asarray(P, np.float32).reshape(-1, 3)
    n = np.where(np.isfinite(nrm).all(axis=1, keepdims=True), nrm, np.array([0.0, 0.0, 1.0])).astype(np.float32)
    out = np.empty((len(P), 6), np.float32)
    out[:, :3] = P + np.float32(delta) * n              # float arithmetic on the float coordinates
    out[:, 3:] = n
    return out


def reference(P, K, r):
    P = np.ascontiguousarray(np.asarray(P, np.float32).reshape(-1, 3))
    key = (P.tobytes(), int(K), float(r))
    if key not in _REF:
        nrm, lists, lam, C = mn.map_normals(P, K, r)
        _REF[key] = Ref(P, int(K), float(r), nrm, lists, lam, C, np.isfinite(nrm).all(axis=1), census_queries(P, nrm))
    return _REF[key]


def case_reference(case):
    return reference(case.points(), case.K, case.r)


def params(K, r, gate=True, iters=3, get_normals=0, tensor_voting=0):
    """The shipped IMLS parameters with LS, in count mode."""
    from planetary_lidar_odometry_amd import config
    p = config.bench_params(iters)
    p.get_normals = get_normals
    p.recompute_normal_count_mode = 1
    p.search_number_normal = int(K)
    p.r_normal = float(r)
    p.normal_angle_constraint = 1 if gate else 0
    p.use_tensor_voting = tensor_voting
    p.tensor_sigma = 1.0            # votes from 0.6 m around a query: the maps here hold 30 points per m²
    return p


def oracle_census(P, K, r, gate=True, get_normals=0):
    """oracle_ctypes.project of the census of map P at the identity pose (get_normals = 1: the same
    queries against the stored normals)."""
    import oracle_ctypes as oc
    ref = reference(P, K, r)
    key = (ref.P.tobytes(), ref.K, ref.r, bool(gate), int(get_normals))
    if key not in _ORACLE:
        _ORACLE[key] = oc.project(np.ascontiguousarray(ref.src.T), np.ascontiguousarray(map_rows(ref.P).T), np.eye(4),
                                  params(K, r, gate, get_normals=get_normals))
    return _ORACLE[key]


def check_against_restatement(ref, n, idx, rej, healthy, label):
    """What a census result (n, idx, rej) — the oracle's on the CPU, the device's on the GPU — owes the
    restatement: the ∞ count, the coverage, and per valid row the normal (healthy: within one float32 ulp
    at 1.0 of float32(restated normal); otherwise ‖C·n‖ within map_normals_np.residual's bound).  Returns
    the largest |difference| to the restated normals (nan where they are not compared)."""
    idx = np.asarray(idx, np.int64)
    n = np.asarray(n, np.float32)
    assert int(rej[REJ_INVALID]) == ref.n_inf, (label, rej, ref.n_inf)
    assert int(np.sum(rej)) + len(idx) == len(ref.P), (label, rej, len(idx))
    assert ref.finite[idx].all(), label
    assert len(idx) >= COVERAGE * int(ref.finite.sum()), (label, len(idx), int(ref.finite.sum()), rej)
    if not len(idx):
        return float("nan")
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() <= 4 * mn.ULP1 and (n[:, 2] >= 0).all(), label
    if healthy:
        err = np.abs(n.astype(np.float64) - ref.nrm[idx].astype(np.float32).astype(np.float64))
        bad = np.nonzero((err > mn.ULP1).any(axis=1))[0]
        assert bad.size == 0, (label, len(bad), idx[bad[:3]], n[bad[:3]], ref.nrm[idx[bad[:3]]])
        return float(err.max())
    res, bound = mn.residual(ref.C[idx], ref.lam[idx], n)
    assert (res <= bound).all(), (label, float((res - bound).max()))
    return float("nan")


def nn1_of_queries(P, src):
    """The NN-1 (no self match: d² > DBL_EPSILON, ties by index) of every census query, brute force."""
    P64 = np.asarray(P, np.float32).astype(np.float64)
    out = np.empty(len(src), np.int64)
    for i, q in enumerate(np.asarray(src, np.float32)[:, :3]):
        d2 = imls_np.exact_d2(q, P64)
        d2 = np.where(d2 > mn.DBL_EPS, d2, np.inf)
        out[i] = int(np.argmin(d2))                     # the first minimum: the lowest index
    return out


def first_copy(P):
    """Per row, the lowest index among its exact copies."""
    _, first, inv = np.unique(np.asarray(P, np.float32) + np.float32(0.0), axis=0, return_index=True, return_inverse=True)
    return first[np.asarray(inv).reshape(-1)]


def sentinel_short_lists(ref):
    """The lists that normals.hip's sentinel test written `j < KC − K − 1` leaves (one sentinel too few:
    a capacity of K + 1 where K < KC, nothing changed at K = KC): the list keeps the K + 1 best, the
    moments read its last K slots — neighbours 2 … K + 1 — and a point with exactly K neighbours counts
    K − 1 in those slots: ∞.  (One sentinel too many, `j ≤ KC − K`, counts the sentinel's −1 as a found
    slot and reads map row −1: out of bounds, so that direction is judged by reading only.)"""
    if ref.K in KC_RUNGS:
        return [np.array(li) for li in ref.lists]
    longer = mn.neighbour_lists(ref.P, ref.K + 1, ref.r)
    return [li[1:] if len(li) == ref.K + 1 else li[:0] for li in longer]


# ---- map kinds: every way of changing the map under count mode ---------------------------------------------
KIND_K, KIND_R, KIND_QUEUE = 6, 1.0, 3
KIND_VOXEL = dict(voxel_size=0.5, max_per_voxel=20, max_range=8.0)


def tilted(P, roll_deg, t=(0.0, 0.0, 0.0)):
    """(M, 6) float32 rows of P rotated about x by roll_deg and moved by t (model_restatement.pose_cloud)."""
    import model_restatement as mr
    return mr.pose_cloud(map_rows(P), mr.make_pose(roll=np.radians(roll_deg), t=t))


@functools.lru_cache(maxsize=None)
def kind_inputs():
    """The clouds and poses of test_gpu_map_normals.py's map-kind sequence.  Every stage's surface has a
    tilt of its own (the lattice: its z pattern), so that no normal of one stage's map is a normal of the
    previous one's: normals left over from the map before cannot pass for the map after."""
    import model_restatement as mr
    centred = plane(600, 4.0, 11) - np.float32([2.0, 2.0, 0.0])
    host = tilted(centred, 0.0)
    host = np.concatenate([host[:7], np.full((2, 6), np.nan, np.float32), host[7:]])     # renumbers the rows behind
    lat = map_rows(lattice())
    return dict(
        host=host,
        device=tilted(plane(600, 4.0, 12), 30.0),
        runs=[lat[:200], lat[200:390], lat[390:]],
        posed_scan=map_rows(plane(600, 4.0, 13)), posed_pose=mr.make_pose(roll=np.radians(-30.0), t=(1.0, -2.0, 0.5)),
        rebase_pose=mr.make_pose(yaw=0.3, roll=np.radians(50.0), t=(-3.0, 1.0, 0.25)),
        voxel_scan1=tilted(centred, 40.0), voxel_pose1=np.eye(4),
        # the second update's sensor is 30 m away: the first update's rows fall out of range (8 m)
        voxel_scan2=map_rows(plane(600, 4.0, 14) - np.float32([2.0, 2.0, 0.0])),
        voxel_pose2=mr.make_pose(roll=np.radians(-20.0), t=(30.0, 0.0, 0.0)),
    )


def finite_points(rows):
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    return np.ascontiguousarray(rows[np.isfinite(rows[:, :3]).all(axis=1)][:, :3])


@functools.lru_cache(maxsize=None)
def kind_maps():
    """[(stage, expected map (M, 3) float32)] in the order the GPU test reaches them, from the suite's
    restatements (model_restatement.pose_cloud, voxel_map_np.update)."""
    import model_restatement as mr
    import voxel_map_np as vm
    g = kind_inputs()
    posed = mr.pose_cloud(g["posed_scan"], g["posed_pose"])
    v1, _ = vm.update(np.zeros((0, 6), np.float32), g["voxel_scan1"], g["voxel_pose1"], **KIND_VOXEL)
    v2, _ = vm.update(v1, g["voxel_scan2"], g["voxel_pose2"], **KIND_VOXEL)
    out = [("host", finite_points(g["host"])), ("device", finite_points(g["device"])),
           ("fifo", finite_points(np.concatenate(g["runs"]))), ("posed", finite_points(posed)),
           ("rebased", finite_points(mr.pose_cloud(posed, g["rebase_pose"]))), ("voxel1", finite_points(v1)),
           ("voxel2", finite_points(v2))]
    # map_clear, then a new map of the size of the one before it
    out.append(("cleared", finite_points(tilted(plane(len(out[-1][1]), 4.0, 15), 10.0))))
    return out


# ---- batches --------------------------------------------------------------------------------------------
BATCH_K, BATCH_R, BATCH_ITERS = 9, 1.0, 4


def batch_maps():
    """Three maps of different sizes (one below a block of 128) for one fused register_frames call."""
    return [pyramid(1500), pyramid(700, 2.5), pyramid(100, 0.8)]


def failed_batch_maps():
    """(A's earlier map, A's current map — the same size, another tilt —, B's map)."""
    return finite_points(tilted(pyramid(700, 2.5, 21), 25.0)), pyramid(700, 2.5, 22), pyramid(500, 2.0, 23)


def registration_source(P, K=BATCH_K, r=BATCH_R):
    """The census queries of map P moved by a small pose: a frame the ICP has something to do with."""
    import model_restatement as mr
    return mr.pose_cloud(reference(P, K, r).src, mr.make_pose(yaw=0.01, pitch=-0.004, t=(0.03, -0.02, 0.015)))


def plate_tensors(P, K=BATCH_K, r=BATCH_R):
    """(M, 6) float32 tensors I − n·nᵀ (xx, xy, xz, yy, yz, zz) of the restated normals ((0, 0, 1) for ∞):
    the voted tensor's eigenvector of the smallest |λ| — what the matcher takes for the normal — is then
    close to the surface normal."""
    n = census_queries(P, reference(P, K, r).nrm)[:, 3:].astype(np.float64)
    return np.stack([1 - n[:, 0] * n[:, 0], -n[:, 0] * n[:, 1], -n[:, 0] * n[:, 2], 1 - n[:, 1] * n[:, 1],
                     -n[:, 1] * n[:, 2], 1 - n[:, 2] * n[:, 2]], axis=1).astype(np.float32)
