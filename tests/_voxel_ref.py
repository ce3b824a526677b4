"""numpy reference of symmicp_ctx_voxel_downsample with exactly the device's arithmetic (include/symmicp.h, DESIGN.md 4
"Voxel downsampling"): every op in float32, keys from the box's floor cells, a stable sort, per-voxel sums taken one point at a
time in ascending row order (rounds over member rank, never np.sum: that one is pairwise), one correctly rounded division per
component, normals divided by the float32 sqrt of (sx*sx + sy*sy) + sz*sz."""
import numpy as np

F = np.float32


class GridError(ValueError):
    """the cases the library answers with SYMMICP_ERR_ARG"""


def grid(xyz, leaf):
    """-> (inv, lo [3] int64, dims [3] int64): the host's grid set-up"""
    xyz = np.asarray(xyz, F)
    leaf = F(leaf)
    if not (np.isfinite(leaf) and leaf > 0):
        raise GridError("leaf must be finite and > 0")
    if not np.all(np.isfinite(xyz)):
        raise GridError("non-finite coordinates")
    inv = F(1) / leaf
    with np.errstate(over="ignore", invalid="ignore"):
        flo = np.floor(xyz.min(axis=0) * inv)
        fhi = np.floor(xyz.max(axis=0) * inv)
    lim = F(2147483648.0)
    if not (np.all(flo >= -lim) and np.all(flo < lim) and np.all(fhi >= -lim) and np.all(fhi < lim)):
        raise GridError("leaf size too small: voxel indices overflow an int32")
    lo = flo.astype(np.int64)
    dims = fhi.astype(np.int64) - lo + 1
    if int(dims[0]) * int(dims[1]) * int(dims[2]) > 2 ** 32:
        raise GridError("leaf size too small: more than 2^32 voxels")
    return inv, lo, dims


def keys(xyz, leaf):
    """the linear voxel key of every point (x fastest, z slowest), int64"""
    xyz = np.asarray(xyz, F)
    inv, lo, dims = grid(xyz, leaf)
    cell = np.floor(xyz * inv).astype(np.int64) - lo
    return cell[:, 0] + dims[0] * (cell[:, 1] + dims[1] * cell[:, 2])


def _seq_sums(vals, first, count):
    """for every voxel v: vals[first[v]] + vals[first[v] + 1] + ... one float32 add at a time, left to right.  vals [n, c]."""
    m = len(first)
    acc = np.zeros((m, vals.shape[1]), F)
    order = np.argsort(-count, kind="stable")              # voxels by count, descending: the active ones are a prefix
    f_o, c_o = first[order], count[order]
    out = np.zeros_like(acc)
    active = m
    r = 0
    while active > 0:
        while active > 0 and c_o[active - 1] <= r:
            active -= 1
        if active == 0:
            break
        if active == 1:
            # one voxel left: finish it with a sequential float32 accumulate from the running value
            rest = vals[f_o[0] + r: f_o[0] + c_o[0]]
            acc[0] = np.add.accumulate(np.concatenate([acc[:1], rest]), axis=0, dtype=F)[-1]
            break
        acc[:active] = acc[:active] + vals[f_o[:active] + r]
        r += 1
    out[order] = acc
    return out


def voxel_downsample(xyz, leaf, nrm=None, min_points=1):
    """-> dict(xyz [m,3], nrm [m,3] or None, count [m] int32, voxel_of [n] int32), as the library returns it"""
    xyz = np.asarray(xyz, F)
    n = xyz.shape[0]
    if min_points < 1:
        raise GridError("min_points must be >= 1")
    k = keys(xyz, leaf)
    rows = np.argsort(k, kind="stable")
    ks = k[rows]
    head = np.ones(n, bool)
    head[1:] = ks[1:] != ks[:-1]
    first = np.flatnonzero(head)
    count = np.diff(np.append(first, n))
    kept = count >= min_points
    out_id = np.full(len(first), -1, np.int64)
    out_id[kept] = np.arange(int(kept.sum()))
    vid = np.cumsum(head) - 1
    voxel_of = np.empty(n, np.int32)
    voxel_of[rows] = out_id[vid]
    first, count = first[kept], count[kept]
    sums = _seq_sums(xyz[rows], first, count)
    mean = sums / count.astype(F)[:, None]
    res = dict(xyz=mean.astype(F), nrm=None, count=count.astype(np.int32), voxel_of=voxel_of)
    if nrm is not None:
        s = _seq_sums(np.asarray(nrm, F)[rows], first, count)
        len2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        pos = len2 > 0
        out = np.zeros_like(s)
        out[pos] = s[pos] / np.sqrt(len2[pos])[:, None]
        res["nrm"] = out
    return res
