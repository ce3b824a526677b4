"""fp64 numpy restatement of the pose-graph optimiser (include/symmicp.h, "multiway registration"): the edge error and its log, the
line-process weights, the cost, the blocks of the first-order linearisation, a dense solve (and a block-Jacobi PCG with the device's
stop rule, for the tolerance measurement), the retraction and the Levenberg-Marquardt loop with the header's control rules.
Independent of the library.  An edge is a tuple (s, t, uncertain, T [4,4], L [6,6])."""
import numpy as np

SMALL2 = 1e-8           # the series of log and exp are used below this squared size (|v|^2 of the log, |w|^2 of the exp)


def inv_rigid(X):
    X = np.asarray(X, np.float64)
    Y = np.eye(4)
    Y[:3, :3] = X[:3, :3].T
    Y[:3, 3] = -X[:3, :3].T @ X[:3, 3]
    return Y


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def log_rot(R):
    """rotation vector of R, angle in [0, pi]: the header's formula"""
    R = np.asarray(R, np.float64)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = min(1.0, max(-1.0, 0.5 * ((R[0, 0] + R[1, 1] + R[2, 2]) - 1.0)))
    s2 = v @ v
    if s2 >= SMALL2:
        s = np.sqrt(s2)
        return v * (np.arctan2(s, c) / s)
    if c > 0.0:
        return v * (1.0 + s2 / 6.0 + 3.0 * s2 * s2 / 40.0)
    # near pi: the axis from the symmetric part, signed by v
    th = np.arctan2(np.sqrt(s2), c)
    d = np.array([R[0, 0], R[1, 1], R[2, 2]])
    i = int(np.argmax(d))
    a = np.zeros(3)
    a[i] = np.sqrt(max((d[i] - c) / (1.0 - c), 0.0))
    for j in range(3):
        if j != i:
            a[j] = (R[i, j] + R[j, i]) / (2.0 * (1.0 - c) * a[i])
    if a @ v < 0.0:
        a = -a
    return th * a


def exp_rot(w):
    w = np.asarray(w, np.float64)
    t2 = w @ w
    if t2 < SMALL2:
        A = 1.0 - t2 / 6.0 + t2 * t2 / 120.0
        B = 0.5 - t2 / 24.0 + t2 * t2 / 720.0
    else:
        t = np.sqrt(t2)
        A = np.sin(t) / t
        B = (1.0 - np.cos(t)) / t2
    K = hat(w)
    return np.eye(3) + A * K + B * (K @ K)


def exp_pose(d):
    """Exp(delta) = [exp([w]x) tau; 0 1]"""
    X = np.eye(4)
    X[:3, :3] = exp_rot(d[:3])
    X[:3, 3] = d[3:]
    return X


def edge_E(Xs, Xt, T, variant=0):
    if variant:
        return inv_rigid(Xt) @ (np.asarray(Xs, np.float64) @ inv_rigid(T))
    return (inv_rigid(Xt) @ np.asarray(Xs, np.float64)) @ inv_rigid(T)


def edge_error(Xs, Xt, T, variant=0):
    E = edge_E(Xs, Xt, T, variant)
    return np.concatenate([log_rot(E[:3, :3]), E[:3, 3]])


def adjoint(T):
    T = np.asarray(T, np.float64)
    A = np.zeros((6, 6))
    A[:3, :3] = T[:3, :3]
    A[3:, 3:] = T[:3, :3]
    A[3:, :3] = hat(T[:3, 3]) @ T[:3, :3]
    return A


def sym_upper(L):
    """the symmetric matrix whose upper triangle is L's"""
    L = np.asarray(L, np.float64).reshape(6, 6)
    U = np.triu(L)
    return U + np.triu(L, 1).T


def line_weight(mu, c):
    t = mu / (mu + c)
    return t * t


def derive_mu(edges, max_dist, preference=1.0):
    return preference * (max_dist * max_dist) * (sum(float(np.asarray(e[4]).reshape(36)[35]) for e in edges) / len(edges))


def quad(L, e, variant=0):
    if variant:
        s = 0.0
        for i in range(5, -1, -1):
            for j in range(5, -1, -1):
                s += e[i] * L[i, j] * e[j]
        return s
    return float(e @ (L @ e))


def assemble(poses, edges, ref, mu, variant=0):
    """everything one pass defines at the poses: e [m,6], c [m], l [m], cost, g [n,6], the dense H [6n,6n] (all nodes) and hdiag [n,6,6];
    the rows of the reference node are zero in g and hdiag.  variant = 1: the same formulas in another association and the reverse
    summation order (for the tolerance measurement)."""
    n, m = len(poses), len(edges)
    e, c, l = np.zeros((m, 6)), np.zeros(m), np.zeros(m)
    g, H = np.zeros((n, 6)), np.zeros((6 * n, 6 * n))
    terms = []
    order = range(m - 1, -1, -1) if variant else range(m)
    for k in order:
        s, t, unc, T, L = edges[k]
        L = sym_upper(L)
        e[k] = edge_error(poses[s], poses[t], T, variant)
        c[k] = quad(L, e[k], variant)
        l[k] = line_weight(mu, c[k]) if unc else 1.0
        terms.append(mu * c[k] / (mu + c[k]) if unc else c[k])
        W = l[k] * L
        A = adjoint(T)
        We = W @ e[k]
        ss, tt = slice(6 * s, 6 * s + 6), slice(6 * t, 6 * t + 6)
        if variant:
            H[ss, ss] += A.T @ (W @ A)
            H[ss, tt] -= (W @ A).T
            H[tt, ss] -= W @ A
        else:
            H[ss, ss] += (A.T @ W) @ A
            H[ss, tt] -= A.T @ W
            H[tt, ss] -= (A.T @ W).T
        H[tt, tt] += W
        g[s] += A.T @ We
        g[t] -= We
    cost = 0.0
    for v in terms:
        cost += v
    g[ref] = 0.0
    hdiag = np.stack([H[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n)])
    hdiag[ref] = 0.0
    return dict(e=e, c=c, l=l, cost=cost, g=g, H=H, hdiag=hdiag)


def cost(poses, edges, mu):
    F = 0.0
    for s, t, unc, T, L in edges:
        e = edge_error(poses[s], poses[t], T)
        c = quad(sym_upper(L), e)
        F += mu * c / (mu + c) if unc else c
    return F


def free_rows(n, ref):
    return np.array([6 * i + a for i in range(n) if i != ref for a in range(6)])


def solve_dense(H, g, lam, ref):
    """(H + lam I) delta = -g over the free nodes -> delta [n,6] (the reference row zero)"""
    n = len(g)
    f = free_rows(n, ref)
    A = H[np.ix_(f, f)] + lam * np.eye(len(f))
    d = np.zeros(6 * n)
    d[f] = np.linalg.solve(A, -g.reshape(-1)[f])
    return d.reshape(n, 6)


def solve_pcg(H, g, lam, ref, tol=1e-10, max_iter=0):
    """block-Jacobi preconditioned CG with the device's rule: stop at r.r <= tol^2 b.b or after max_iter (0: 6 (n - 1)) iterations
    -> (delta [n,6], iterations, relative residual)"""
    n = len(g)
    f = free_rows(n, ref)
    A = H[np.ix_(f, f)] + lam * np.eye(len(f))
    b = -g.reshape(-1)[f]
    nb = len(f) // 6
    Minv = [np.linalg.inv(A[6 * i:6 * i + 6, 6 * i:6 * i + 6]) for i in range(nb)]
    prec = lambda r: np.concatenate([Minv[i] @ r[6 * i:6 * i + 6] for i in range(nb)])
    x, r = np.zeros_like(b), b.copy()
    bb = b @ b
    it, rr = 0, bb
    if bb > 0.0:
        z = prec(r)
        p, rz = z.copy(), r @ z
        for it in range(1, (max_iter or 6 * (n - 1)) + 1):
            Ap = A @ p
            a = rz / (p @ Ap)
            x += a * p
            r -= a * Ap
            rr = r @ r
            if rr <= tol * tol * bb:
                break
            z = prec(r)
            rz, rz0 = r @ z, rz
            p = z + (rz / rz0) * p
    d = np.zeros(6 * n)
    d[f] = x
    return d.reshape(n, 6), it, (np.sqrt(rr / bb) if bb > 0.0 else 0.0)


def retract(poses, delta, ref):
    out = np.array(poses, np.float64).copy()
    for i in range(len(out)):
        if i != ref:
            out[i] = out[i] @ exp_pose(delta[i])
            out[i][3] = (0.0, 0.0, 0.0, 1.0)
    return out


def optimize(poses, edges, ref=0, mu=None, max_dist=None, preference=1.0, max_iterations=100, min_relative_decrease=1e-6,
             min_increment=1e-9, prune_threshold=0.25, solver=solve_dense, variant=0):
    """the LM loop with the header's control rules; one iteration = one linearisation, one solve, one trial"""
    X = np.array(poses, np.float64).copy()
    n = len(X)
    if mu is None:
        mu = derive_mu(edges, max_dist, preference)
    lam, nu = None, 2.0
    its = acc = 0
    reason = 1
    F0 = Fc = None
    trace = []
    while True:
        a = assemble(X, edges, ref, mu, variant)
        F = a["cost"]
        if F0 is None:
            F0 = Fc = F
        if lam is None:
            lam = 1e-5 * max(a["hdiag"][i][k, k] for i in range(n) for k in range(6))
        d = solver(a["H"], a["g"], lam, ref)
        Xn = retract(X, d, ref)
        Fn = cost(Xn, edges, mu)
        model = float((d * (lam * d - a["g"])).sum())
        dmax = float(np.abs(d).max())
        its += 1
        ok = Fn < F
        trace.append(dict(cost=F, cost_trial=Fn, lam=lam, accepted=ok, delta_max=dmax, grad_max=float(np.abs(a["g"]).max())))
        stop = False
        if ok:
            rho = (F - Fn) / model
            lam, nu = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 2.0
            X, Fc = Xn, Fn
            acc += 1
            if F - Fn <= min_relative_decrease * F:
                stop, reason = True, 2
        else:
            lam, nu = lam * nu, 2.0 * nu
        if not stop and dmax <= min_increment:
            stop, reason = True, 3
        if not stop and its >= max_iterations:
            stop, reason = True, 1
        if stop:
            break
    fin = assemble(X, edges, ref, mu)
    unc = np.array([bool(e[2]) for e in edges])
    return dict(poses=X, iterations=its, accepted=acc, stop_reason=reason, cost_initial=F0, cost_final=Fc, mu=mu, lam=lam,
                weights=fin["l"], pruned=unc & (fin["l"] < prune_threshold), trace=trace)


# ---- graphs for the tests -------------------------------------------------------------------------------------------------------
def random_pose(rng, rot=1.0, trans=1.0):
    w = rng.normal(size=3)
    w *= rng.uniform(0.0, rot) / np.linalg.norm(w)
    X = np.eye(4)
    X[:3, :3] = exp_rot(w)
    X[:3, 3] = rng.uniform(-trans, trans, 3)
    return X


def random_information(rng, npts=40, spread=1.0):
    """Open3D's information matrix of npts random target points (sum G^T G, rotation first)"""
    q = rng.uniform(-spread, spread, (npts, 3))
    L = np.zeros((6, 6))
    for x, y, z in q:
        G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1.0]])
        L += G.T @ G
    return L


def relative(Xs, Xt):
    """the T of an edge s -> t consistent with the poses: X_t^-1 X_s"""
    return inv_rigid(Xt) @ Xs


def make_graph(rng, n, pairs, rot=1.0, trans=1.0, noise=0.0, npts=40):
    """true poses [n,4,4] and the edges of `pairs` (s, t, uncertain) with T = X_t^-1 X_s turned by a random pose of size `noise`"""
    truth = np.stack([random_pose(rng, rot, trans) for _ in range(n)])
    edges = []
    for s, t, unc in pairs:
        T = relative(truth[s], truth[t])
        if noise:
            T = T @ random_pose(rng, noise, noise)
        edges.append((int(s), int(t), int(unc), T, random_information(rng, npts)))
    return truth, edges


def perturb(rng, poses, ref, size):
    out = np.array(poses, np.float64).copy()
    for i in range(len(out)):
        if i != ref:
            out[i] = out[i] @ random_pose(rng, size, size)
    return out


def ring_pairs(n):
    return [(i, (i + 1) % n, 0 if i + 1 < n else 1) for i in range(n)]


# ---- the graphs of the pass probe (tests/test_gpu_posegraph.py) and the tolerance measurement ---------------------------------------
PASS_MU = 1.0                # l of the probes' uncertain edges spreads over (0, 1) at this mu
PASS_LAMBDA_REL = 1e-5       # lambda of the probes = this * the largest diagonal entry of H (the loop's lambda_0)
# cg_max_iterations of the probes (0: the default 6 (n - 1)).  The 65-chain's system has a condition number of 8.5e4 and its PCG needs 626
# iterations in fp64 for 1e-10; at the default 384 it stops at a residual of 6.7e-7, where two roundings of the same solve are 2.8e-4
# apart.  The probe compares converged solves, so it lifts the cap there.
PASS_CG_MAX = {"chain65": 2000}


def _probe(seed, n, pairs, ref, wrong=()):
    """poses = the truth (rotations up to 0.5 rad, so edge rotations up to about 1 rad) perturbed by 0.1; T with noise 0.05; the
    uncertain edges listed in `wrong` turned by 0.5 rad more: |w_E| stays far below 3"""
    rng = np.random.default_rng(seed)
    truth, edges = make_graph(rng, n, pairs, rot=0.5, trans=2.0, noise=0.05)
    for k in wrong:
        s, t, unc, T, L = edges[k]
        edges[k] = (s, t, unc, T @ random_pose(rng, 0.5, 0.2), L)
    return perturb(rng, truth, ref, 0.1), edges, ref


def chain_plus_closures(seed, n, m):
    rng = np.random.default_rng(seed)
    pairs = [(i, i + 1, 0) for i in range(n - 1)]
    while len(pairs) < m:
        s, t = (int(v) for v in rng.integers(0, n, 2))
        if s != t:
            pairs.append((s, t, 1))
    return pairs


def pass_graphs(with_cap=False):
    """name -> (poses, edges, ref)"""
    seven = [(0, 1, 0), (1, 2, 0), (1, 2, 1), (2, 3, 0), (3, 2, 1), (3, 4, 0), (4, 5, 0), (5, 6, 0), (6, 1, 1), (2, 5, 1), (4, 1, 1), (6, 3, 1)]
    star = [((0, i, i % 3 == 0) if i % 2 else (i, 0, i % 3 == 0)) for i in range(1, 130)]
    g = {
        "pair": _probe(11, 2, [(0, 1, 0)], 0),
        "ring3": _probe(12, 3, [(0, 1, 0), (1, 2, 0), (2, 0, 1)], 0),
        "seven": _probe(13, 7, seven, 6, wrong=(9,)),          # node 0 has degree 1; 1 -> 2 twice; 2 -> 3 and 3 -> 2; reference = last
        "chain65": _probe(14, 65, [(i, i + 1, 0) for i in range(64)], 0),
        "star130": _probe(15, 130, star, 5, wrong=(2, 8)),     # the hub is free and has degree 129
        "n100": _probe(16, 100, chain_plus_closures(16, 100, 257), 3, wrong=(120, 200, 250)),
    }
    if with_cap:
        g["cap"] = _probe(17, 1024, chain_plus_closures(17, 1024, 16384), 0, wrong=tuple(range(2000, 16384, 1000)))
    return g


def turned(T, degrees):
    """T followed on the source side by a turn about z: a plausible but wrong registration"""
    W = np.eye(4)
    W[:3, :3] = exp_rot(np.array([0.0, 0.0, np.radians(degrees)]))
    return T @ W


RING_MAX_DIST = 0.05


def ring_cases():
    """name -> (start poses, edges, truth) of the optimiser tests, reference node 0, mu derived from RING_MAX_DIST:
    consistent  a ring of 8 with exact T (the closure 7 -> 0 uncertain), started 0.05 off the truth
    noisy       the same ring with T noise 0.01 and a true closure 2 -> 6
    false       noisy plus the closure 1 -> 5 whose T is the true one turned by 30 degrees (the last edge)"""
    out = {}
    rng = np.random.default_rng(21)
    truth, edges = make_graph(rng, 8, ring_pairs(8))
    out["consistent"] = (perturb(rng, truth, 0, 0.05), edges, truth)
    rng = np.random.default_rng(22)
    truth, edges = make_graph(rng, 8, ring_pairs(8) + [(2, 6, 1)], noise=0.01)
    start = perturb(rng, truth, 0, 0.05)
    out["noisy"] = (start, edges, truth)
    L = random_information(rng)
    out["false"] = (start, edges + [(1, 5, 1, turned(relative(truth[1], truth[5]), 30.0), L)], truth)
    return out


def relerr(a, b):
    """max |a - b| relative to the largest |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def measure(with_cap=False):
    """the spreads the test tolerances are 100 x of: the same formulas in another association and summation order; for delta the
    device's PCG against the dense solve, and the dense solve of the other order's (H, g) against it (what rounding alone does to the
    solution of each system)"""
    worst_f, worst_d = 0.0, 0.0
    for name, (poses, edges, ref) in pass_graphs(with_cap).items():
        a, b = assemble(poses, edges, ref, PASS_MU), assemble(poses, edges, ref, PASS_MU, variant=1)
        lam = PASS_LAMBDA_REL * max(a["hdiag"][i][k, k] for i in range(len(poses)) for k in range(6))
        sf = max(relerr(b[k], a[k]) for k in ("e", "c", "l", "g", "hdiag"))
        sf = max(sf, abs(a["cost"] - b["cost"]) / a["cost"])
        dd = solve_dense(a["H"], a["g"], lam, ref)
        dp, it, res = solve_pcg(a["H"], a["g"], lam, ref, max_iter=PASS_CG_MAX.get(name, 0))
        sd, so = relerr(dp, dd), relerr(solve_dense(b["H"], b["g"], lam, ref), dd)
        print("%-8s n %4d m %5d  order spread %.2e   delta: pcg vs dense %.2e (%d iterations, residual %.1e), dense of the other order vs dense %.2e" % (
            name, len(poses), len(edges), sf, sd, it, res, so))
        worst_f, worst_d = max(worst_f, sf), max(worst_d, sd, so)
    print("worst: %.2e %.2e" % (worst_f, worst_d))
    pcg = lambda H, g, lam, ref: solve_pcg(H, g, lam, ref)[0]
    for name, (start, edges, truth) in ring_cases().items():
        a = optimize(start, edges, max_dist=RING_MAX_DIST)
        print("%-10s dense: %d iterations (%d accepted, reason %d), cost %.6g -> %.6g" % (
            name, a["iterations"], a["accepted"], a["stop_reason"], a["cost_initial"], a["cost_final"]))
        for what, b in (("the PCG", optimize(start, edges, max_dist=RING_MAX_DIST, solver=pcg)),
                        ("the other order", optimize(start, edges, max_dist=RING_MAX_DIST, variant=1))):
            print("    with %s: %d iterations, max |dX| %.2e, |dF| %.2e (relative %.2e), weight spread %.2e" % (
                what, b["iterations"], np.abs(a["poses"] - b["poses"]).max(), abs(a["cost_final"] - b["cost_final"]),
                abs(a["cost_final"] - b["cost_final"]) / max(a["cost_final"], 1e-300), np.abs(a["weights"] - b["weights"]).max()))


if __name__ == "__main__":
    import sys
    measure("cap" in sys.argv[1:])
