"""The frames, fixtures and parameters of the cloud-operation frame tests (test_cloud_frames_ref.py on the CPU, test_gpu_cloud_frames.py
on the GPU), what the numpy references count of exact ties in them, and what a run in another unit of length must equal.

Frames: a power-of-two unit s (cloud x s: exact), and an offset o extents from the origin -- _frame_cases' construction for one cloud:
off = o E (1, -0.7, 0.3) with E the largest extent of the cloud's bounding box, added in fp64 and rounded to fp32, normals untouched
(the cat pair goes through _frame_cases.shifted itself: E of the pair, which is the cat source's).  The nominal frames are FAR = 1e3
and 1e4 extents and TIE = 1e5 extents; OFFSETS holds, per fixture, the nearest offsets that meet the conditions below.
Fixtures (all in the tree): the cat source with its golden normals (3400 rows), the cat pair, _cluster_ref.scene (7850 rows),
_segplane_ref.floor_scene (11 492 rows) and, for the NDT map, the first 8000 rows of the c4 target's sequence (test_gpu_ndt.py's 4000
rows are its first half).

Measured by test_cloud_frames_ref.py, which prints these numbers and asserts the thresholds next to them:

    the cat source, E = 199.06           o = 0     1e3     1e4     1e5   1.05e5
    duplicate rows                           0       0       0     246      260      (FAR: 0; TIE: >= 100)
    rows tied at the k-th d2, k = 10        11       7      23     842      848      (TIE: >= 500 for every k used)
                              k = 16         8       5      19     864      900
                              k = 17        10       7      31     909      893      (the statistical filter's 16 and the row itself)
                              k = 20        10       7      26     878      831
                              k = 21         5       4      28     877      879      (the statistical filter's 20 and the row itself)
    ordered pairs with d2 == r2, r = 2       0       0      14    1628     1626      (TIE: >= 900 for each of r = 2, 4, 6)
                                 r = 4       0       0       6     838      942
                                 r = 6       0       0      20    2748     2472
    FPFH pairs ambiguous at r = 5.53    0.37 %  0.39 %  0.38 %  0.33 %   0.37 %      (<= 1 % in every frame)
  At 1e5 extents the cat is quantised to 2, 1 and 0.5 along x, y and z and r = 4 has 838 boundary pairs, short of 900: the cat's tie
  frame is 1.05e5 extents, the nearest offset tried (in steps of 5e3; 0.95e5 has 908) at which every threshold holds.

    duplicate rows at o =               1e3     8e3     9e3     1e4     1e5
    the cat target (the pair)             0               .       0     214
    the scene, E = 437.32                 0       2       0       2    2973
    the floor scene, E = 431.45           0       0       0       2    4132
    the NDT cloud, E = 1.038              0       0       4       4     681
  so the far frames are 1e3 and 1e4 for the cat and the pair, 1e3 and 9e3 for the two scenes, 1e3 and 8e3 for the NDT cloud.
  The pair at 1e5 extents: 246 / 214 duplicate rows, and 201 source rows whose nearest target rows tie (the lowest row must win).

    the scene at 1e5 extents is quantised to 4, 2 (and its multiples) and 1, so that d2 is a whole number.  eps = 2 spacings (r2 = 7.635)
    has no pair at d2 == r2; TIE_EPS = 3 (r2 = 9) has 4490 ordered pairs there (>= 100).
    the floor scene at 1e5 extents is quantised to 4, 2 and 1.  The scoring measures fp32 offsets of the cloud about its fp32 pivot from
    planes through three such points: at the scene's own max_dist (0.5 spacings) no (evaluated hypothesis, row) pair has
    |offset| == max_dist, at 2 there are 26, at TIE_MAX_DIST = 4 (a multiple of all three quanta) 1468 (>= 100).
"""
import numpy as np

import _cluster_ref as CR
import _frame_cases as FC
import _knn_ref as K
import _segplane_ref as S

f32 = np.float32

UNIT_EXPONENTS = (-10, 10)
FAR = (1e3, 1e4)
TIE = 1e5
# fixture -> (far, far, tie): the nominal frames, or the nearest offsets at which the fixture meets the conditions (the docstring)
OFFSETS = {"cat": (1e3, 1e4, 1.05e5), "pair": FAR + (TIE,), "scene": (1e3, 9e3, TIE), "floor": (1e3, 9e3, TIE), "ndt": (1e3, 8e3, TIE)}
FRAME_NAMES = ("far1", "far2", "tie")
DIRECTION = np.array([1.0, -0.7, 0.3])

KNN_K = (10, 16, 20)             # the k-NN entry takes 3 .. 16: 20 is refused, and that is what its case asserts
KNN_MAX = 16
RADII = (2.0, 4.0, 6.0)          # fl(r) fl(r) is exact for these
FPFH_R = 5.53
SOR = ((16, 1.0), (16, 2.0), (20, 1.0), (20, 2.0))
ROR_R = 4.0
SCENE_EPS = 2 * CR.CAT_SPACING   # test_gpu_cluster.py's scene_ref
SCENE_MIN_POINTS = (1, 4)
TIE_EPS = 3.0                    # eps * eps = 9: a whole number of the scene's d2 quantum at TIE (the docstring's count)
ORIENT_K = (10, 16)
VIEWPOINT = (500.0, -300.0, 80.0)          # test_gpu_orient.py's viewpoint outside the box
DIRECTION_RULE = (0.3, -0.5, -0.8)         # ... and its direction
PLANE_H = 256
TIE_MAX_DIST = 4.0               # a multiple of the floor scene's three quanta at TIE (the docstring's count)
EVAL_QUANTILE = 0.8
NDT_ROWS = 8000
NDT_RES = 0.1                    # test_gpu_ndt.py's RES and test_gpu_ndt_map.py's context test
VOXEL_LEAF = 4.0

# the thresholds of the conditions
MIN_DUPLICATES = 100
MIN_KTH_TIES = 500
MIN_BOUNDARY_PAIRS = 900
MIN_FIXTURE_BOUNDARY = 100
MAX_AMBIGUOUS = 0.01


# ---- frames -------------------------------------------------------------------------------------------------------------------------
def extent(xyz):
    x = np.asarray(xyz, np.float64)
    return float(np.max(x.max(0) - x.min(0)))


def offset_of(xyz, o):
    return o * extent(xyz) * DIRECTION


def shifted(xyz, o):
    """the cloud o extents from the origin (o = 0: the cloud itself) -> (xyz f32, the fp64 offset)"""
    off = offset_of(xyz, o)
    return np.ascontiguousarray((np.asarray(xyz, f32).astype(np.float64) + off).astype(f32)), off


def frame(fixture, xyz, name):
    """the fixture's cloud in its frame `name` of FRAME_NAMES -> (xyz f32, offset)"""
    return shifted(xyz, OFFSETS[fixture][FRAME_NAMES.index(name)])


def shifted_point(p, off):
    """a viewpoint moved with the cloud, as the fp32 values the API receives"""
    return tuple(float(v) for v in (np.asarray(p, np.float64) + off).astype(f32))


def scaled(xyz, e):
    return np.ascontiguousarray(np.asarray(xyz, f32) * f32(2.0 ** e))


def length(v, e=0):
    """a length argument in the unit 2^e: the fp32 value times the fp32 s, as the float the API takes"""
    return float(f32(v) * f32(2.0 ** e))


def lengths(p, e=0):
    return tuple(length(v, e) for v in p)


def shifted_transform(X, off):
    """X rewritten for the frame moved by off, as _frame_cases.shifted rewrites a truth -> fp32 4x4"""
    Xt = np.array(X, np.float64).reshape(4, 4)
    Xt[:3, 3] = Xt[:3, 3] + off - Xt[:3, :3] @ off
    return Xt.astype(f32)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def cat_pair(cat):
    """the session fixture `cat` as a _frame_cases pair"""
    return dict(src=cat["src"], tgt=cat["tgt"], src_n=cat["src_n"], tgt_n=cat["tgt_n"])


def pair_frame(d, name):
    """the pair in its frame `name`, by _frame_cases.shifted"""
    return FC.shifted(d, OFFSETS["pair"][FRAME_NAMES.index(name)])


def scene(cat):
    return CR.scene(cat["src"])


def floor(cat):
    return S.floor_scene(cat["src"])[0]


def ndt_cloud():
    from symmicp import synth
    return np.ascontiguousarray(synth.c4_surface(NDT_ROWS)["tgt"][:NDT_ROWS])


def random_signs(nrm, seed=5):
    """test_gpu_orient.py's catn: the normals under random signs"""
    sign = np.where(np.random.default_rng(seed).random(len(nrm)) < 0.5, -1.0, 1.0).astype(f32)
    return nrm * sign[:, None]


def eval_cases(d, off=None):
    """[(name, X fp32, max_dist)] of a pair: the identity and _frame_cases.nudge (rewritten for the frame moved by off), each at
    max_dist 0 and at the EVAL_QUANTILE quantile of its own neighbour distances (fp32)"""
    import _eval_ref as E
    out = []
    for name, X in (("identity", np.eye(4, dtype=f32)), ("nudge", FC.nudge(d))):
        if off is not None:
            X = shifted_transform(X, off)
        _, d2 = E.nearest(E.move(X, d["src"]), d["tgt"])
        out += [(name, X, 0.0), (name, X, float(f32(np.sqrt(np.quantile(d2.astype(np.float64), EVAL_QUANTILE)))))]
    return out


# ---- what the references say of ties ----------------------------------------------------------------------------------------------------
def duplicate_rows(xyz):
    """rows that share their three coordinates with another row"""
    _, inv, cnt = np.unique(np.asarray(xyz, f32), axis=0, return_inverse=True, return_counts=True)
    return int((cnt[inv.ravel()] > 1).sum())


def kth_ties(d2, k):
    """rows whose k-th and (k+1)-th neighbour (the row itself counted, as the walk counts it) are at bit-equal d2, from the d2 of
    _knn_ref.knn(xyz, k + 1 or more) -> bool [n]"""
    return d2[:, k - 1] == d2[:, k]


def d2_matrix(xyz):
    """the fp32 d2 of every row against every row, in the kernels' association (a few thousand rows)"""
    return K._d2(np.asarray(xyz, f32), np.asarray(xyz, f32))


def boundary_pairs(sets, r):
    """ordered pairs of radius_sets' lists at d2 == fl(r) fl(r)"""
    return int((sets[3] == f32(r) * f32(r)).sum())


def plane_boundary_pairs(xyz, ref, max_dist):
    """(evaluated hypothesis, row) pairs of a _segplane_ref.segment result on xyz whose fp32 offset is exactly max_dist"""
    p = np.ascontiguousarray(xyz, f32) - ref["pivot"]
    md = f32(max_dist)
    return sum(int((np.abs(S.offsets32(p, ref["hyp"][h])) == md).sum()) for h in np.nonzero(ref["hyp_status"] == S.EVALUATED)[0].tolist())


# ---- a run in the unit 2^e (b) against the run in the original unit (a): what both test files assert, of the references and of the device
# Every scaling below is by a power of two and meets no underflow or overflow at 2^+-10 on these fixtures, so it is exact: zero tolerance.
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def times(a, e, power=1):
    """a x s^power in a's own precision (exact)"""
    a = np.asarray(a)
    return a * a.dtype.type(2.0 ** (e * power))


def unit_knn(a, b, e):
    assert np.array_equal(a[0], b[0]), int((a[0] != b[0]).sum())
    assert same_bits(times(a[1], e, 2), b[1])


def unit_radius(a, b, e):
    for u, v in zip(a[:3], b[:3]):                              # counts, offsets, rows
        assert np.array_equal(u, v)
    assert same_bits(times(a[3], e, 2), b[3])


def unit_sor(a, b, e):
    assert np.array_equal(a["rows"], b["rows"])
    assert same_bits(times(np.asarray(a["mean_dist"], np.float64), e), np.asarray(b["mean_dist"], np.float64))
    s = 2.0 ** e
    assert (a["mu"] * s, a["sd"] * s, a["thr"] * s) == (b["mu"], b["sd"], b["thr"]), (a["mu"], a["sd"], a["thr"], b["mu"], b["sd"], b["thr"])


def unit_ror(a, b, e=0):
    assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["neighbors"], b["neighbors"])


def unit_cluster(a, b, e=0):
    assert np.array_equal(a["labels"], b["labels"]) and a["clusters"] == b["clusters"] and np.array_equal(a["sizes"], b["sizes"])
    assert np.array_equal(a["core"], b["core"]) and np.array_equal(a["neighbors"], b["neighbors"])


ORIENT_COUNTS = ("graph_edges", "tree_edges", "components", "largest_component", "flipped", "rounds")


def unit_orient(a, b, e=0):
    assert {k: a[k] for k in ORIENT_COUNTS} == {k: b[k] for k in ORIENT_COUNTS}
    assert np.array_equal(a["flip"], b["flip"]) and np.array_equal(a["component"], b["component"]) and np.array_equal(a["tree"], b["tree"])
    assert same_bits(a["normals"], b["normals"])


def unit_fpfh(a, b, e=0):
    """the weights 1 / d2 scale by the exact power of two s^-2 and the normalisation cancels it: identical bits"""
    assert np.array_equal(a["count"], b["count"]) and same_bits(a["spfh"], b["spfh"]) and same_bits(a["fpfh"], b["fpfh"])


def unit_hypotheses(a, b, e):
    """a, b: (status [H], hyp [H,4] f32, pivot [3] f32)"""
    assert np.array_equal(a[0], b[0]), int((a[0] != b[0]).sum())
    assert same_bits(a[1][:, :3], b[1][:, :3]) and same_bits(times(a[1][:, 3], e), b[1][:, 3])
    assert same_bits(times(a[2], e), b[2])


def unit_segment(a, b, e):
    assert a["status"] == b["status"] == 0
    assert np.array_equal(a["hyp_status"], b["hyp_status"]) and np.array_equal(a["hyp_inliers"], b["hyp_inliers"])
    for key in ("best_hypothesis", "evaluated", "inliers_ransac", "inliers_final", "count"):
        assert a[key] == b[key], key
    assert np.array_equal(a["rows"], b["rows"])
    for key in ("plane", "plane32"):
        assert same_bits(a[key][:3], b[key][:3]) and same_bits(times(a[key][3:], e), b[key][3:]), (key, a[key], b[key])
    assert same_bits(times(a["distance"], e), b["distance"])
    assert a["rmse_final"] * 2.0 ** e == b["rmse_final"]


def unit_eval(a, b, e):
    s = 2.0 ** e
    assert a["inliers"] == b["inliers"] and np.array_equal(a["nn"], b["nn"]) and a["fitness"] == b["fitness"]
    assert same_bits(times(a["d2"], e, 2), b["d2"])                                 # (+Inf stays +Inf)
    assert a["sum_d2"] * s * s == b["sum_d2"] and a["mean_d2"] * s * s == b["mean_d2"] and a["rmse"] * s == b["rmse"]
    assert same_bits(times(np.asarray(a["sum_q"], np.float64), e), np.asarray(b["sum_q"], np.float64))
    assert same_bits(times(np.asarray(a["sum_qq"], np.float64), e, 2), np.asarray(b["sum_qq"], np.float64))
    A, B = np.asarray(a["information"], np.float64), np.asarray(b["information"], np.float64)
    assert same_bits(A[:3, :3] * s * s, B[:3, :3]) and same_bits(A[:3, 3:] * s, B[:3, 3:]) and same_bits(A[3:, :3] * s, B[3:, :3])
    assert same_bits(A[3:, 3:], B[3:, 3:])


def unit_ndt(a, b, e):
    assert np.array_equal(a["key"], b["key"]) and np.array_equal(a["count"], b["count"]) and np.array_equal(a["grid"], b["grid"])
    assert same_bits(times(a["mean"], e), b["mean"]) and same_bits(times(a["cov"], e, 2), b["cov"])
    if "axes" in a:                                             # the device's factors
        assert same_bits(a["axes"], b["axes"]) and same_bits(times(a["inv_eig"], e, -2), b["inv_eig"])
    else:                                                       # the reference's eigh
        assert same_bits(times(a["lam"], e, 2), b["lam"]) and same_bits(times(a["M"], e, -2), b["M"])


def unit_voxel(a, b, e):
    assert np.array_equal(a["voxel_of"], b["voxel_of"]) and np.array_equal(a["count"], b["count"])
    assert same_bits(times(a["xyz"], e), b["xyz"])
    assert (a["nrm"] is None) == (b["nrm"] is None) and (a["nrm"] is None or same_bits(a["nrm"], b["nrm"]))
