"""Time of the pose-graph solver (tsl_pose_graph.hip, mapping.PoseGraph) on the loops of tests/pose_graph_scenes.py: a robot drives n poses round a circle,
the start is its integrated odometry, the closures join the ends of the loop and every tenth pose to the pose a quarter turn on.  The odometry noise is
scaled by sqrt(64 / n), so that the drift at the end of the loop is the same at every size.

  * n = 64, 1 024 and 4 096 with one variant (every edge), the defaults of PoseGraph.solve (20 iterations at the most, pcg_tol 1e-3, pcg_max 1 000);
  * leave-one-out over all closures of the 1 024-pose loop: 1 + closures variants in ONE launch.

Times are medians of REPEATS after WARMUP of HIP events around the asynchronous device call (R, T, Z, L and every output as torch tensors on the device;
the call builds the incidence lists and runs the union-find on the host first, which the events do not see, so the host clock around call +
synchronise is given too).  "per PCG iteration" is the event time over the conjugate-gradient iterations of all variants' reports -- it carries the
linearisations and trial evaluations with it.  Baseline, the loop the call replaces, on the host: the same Levenberg-Marquardt loop (same damping
schedule, same accept / reject, same stops) with a numpy linearisation and scipy.sparse.linalg.spsolve on the assembled matrix in place of the
preconditioned conjugate gradients, run once per variant; medians of 3 at one variant, ONE run of all variants for the leave-one-out.  The two ways solve
the linear systems differently (pcg_tol 1e-3 against a direct solve), so they agree in the final cost to a few digits, not bit for bit: both costs are
printed.  No threshold is set.  Writes the table to --out (default profiles/pose_graph.txt) and prints it.  One process; run it under `timeout`."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

import pose_graph_ref as ref
import pose_graph_scenes as sc
from taichislam_amd.mapping import PoseGraph
from taichislam_amd.mapping.pose_graph import REPORT_DTYPE, edge_masks

WARMUP, REPEATS = 2, 7
SIZES = (64, 1024, 4096)
LOO_SIZE = 1024
O = dict(ref.DEFAULTS)


def scene(n):
    s = (64.0 / n) ** 0.5
    return sc.loop(n, seed=n, odo_t=0.02 * s, odo_r=0.01 * s)


def event_ms(fn, torch, repeats=REPEATS):
    """median and least time of fn between two events on the current stream, and the median host time of fn + synchronise"""
    ms, host = [], []
    for i in range(WARMUP + repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            ms.append(a.elapsed_time(b))
            host.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms), statistics.median(host)


def host_lm(G, on):
    """(final cost, outer iterations, status) of the Levenberg-Marquardt loop with a sparse direct solve"""
    R, T = G["R"].copy(), G["T"].copy()
    N, ij, L = len(R), G["ij"][on], ref.full(G["L"][on], 1.0)
    Z = G["Z"][on]
    a, b = ij[:, 0], ij[:, 1]
    free = np.flatnonzero(np.repeat(G["fixed"] == 0, 6))
    rows = (6 * np.stack([a, b, a, b], 1)[:, :, None, None] + np.arange(6)[None, None, :, None] + np.zeros((1, 1, 1, 6), np.int64)).reshape(-1)
    cols = (6 * np.stack([a, b, b, a], 1)[:, :, None, None] + np.arange(6)[None, None, None, :] + np.zeros((1, 1, 6, 1), np.int64)).reshape(-1)

    def cost_at(R, T):
        r, den = ref.residual(R[a], T[a], R[b], T[b], Z)
        return r, float(np.einsum("ei,eij,ej->", r, L, r)), bool((den < 1.0).any())
    damping, status, n_it = O["damping"], 1, 0
    r, cost, _ = cost_at(R, T)
    for _ in range(O["iters"]):
        n_it += 1
        Ri = R[b].transpose(0, 2, 1)
        ti = -np.einsum("eij,ej->ei", Ri, T[b])
        hat = np.zeros((len(b), 3, 3))
        hat[:, 0, 1], hat[:, 0, 2], hat[:, 1, 0], hat[:, 1, 2], hat[:, 2, 0], hat[:, 2, 1] = -ti[:, 2], ti[:, 1], ti[:, 2], -ti[:, 0], -ti[:, 1], ti[:, 0]
        A = np.zeros((len(b), 6, 6))
        A[:, :3, :3], A[:, 3:, 3:], A[:, :3, 3:] = Ri, Ri, hat @ Ri
        W = np.einsum("eki,ekl,elj->eij", A, L, A)
        q = np.einsum("eki,ekl,el->ei", A, L, r)
        H = sp.coo_matrix((np.stack([W, W, -W, -W], 1).reshape(-1), (rows, cols)), shape=(6 * N, 6 * N)).tocsc()
        g = np.zeros(6 * N)
        np.add.at(g, (6 * a[:, None] + np.arange(6)).reshape(-1), q.reshape(-1))
        np.add.at(g, (6 * b[:, None] + np.arange(6)).reshape(-1), -q.reshape(-1))
        H = H + sp.diags(damping * H.diagonal())
        x = np.zeros(6 * N)
        x[free] = spsolve(H[free][:, free], -g[free])
        x = x.reshape(N, 6)
        Rt, Tt = ref.retract(x, R, T)
        rt, trial, flipped = cost_at(Rt, Tt)
        step = float(np.sqrt((x * x).sum(1).max()))
        if not flipped and np.isfinite(trial) and trial < cost:
            dec = cost - trial
            R, T, r = Rt, Tt, rt
            damping = max(damping / O["damping_down"], O["damping_min"])
            stop = step < O["min_step"] or dec <= O["rel_tol"] * cost
            cost = trial
            if stop:
                status = 0
                break
        else:
            damping *= O["damping_up"]
            if damping > O["damping_max"]:
                status = 2
                break
    return cost, n_it, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_graph: no GPU")
    dev = torch.device("cuda:0")
    lines = [f"tools/bench_pose_graph.py: medians of {REPEATS} after {WARMUP} warm-up calls; one MI355X, one process",
             "event = HIP events on the current stream around the asynchronous device call; host = the host clock around call + synchronise (it adds the incidence lists "
             "and the union-find the call makes on the host); per PCG iteration = event time / the conjugate-gradient iterations of all variants",
             "baseline = the same Levenberg-Marquardt loop on the host, numpy linearisation + scipy.sparse.linalg.spsolve, once per variant (one variant: median of 3; "
             "leave-one-out: one run of all variants)"]

    def put(s):
        lines.append(s)
        print(s, flush=True)

    def run(tag, G, masks):
        N, E = len(G["R"]), len(G["ij"])
        B = 1 if masks is None else len(masks)
        pg = PoseGraph(N, E, B)
        t = {k: torch.from_numpy(np.ascontiguousarray(G[k], dtype=np.float64)).to(dev) for k in ("R", "T", "Z", "L")}
        words = None if masks is None else edge_masks(masks)
        out = {}

        def call():
            out["o"] = pg.solve(t["R"], t["T"], G["fixed"], G["ij"], t["Z"], t["L"], masks=words)
        med, least, host = event_ms(call, torch)
        rep = PoseGraph.decode(out["o"]["report"])
        pcg = int(sum(int(r["it"]["pcg_iters"][:r["iterations"]].sum()) for r in rep))
        its = [int(r["iterations"]) for r in rep]
        reps = 3 if B == 1 else 1
        bt, base = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            base = [host_lm(G, np.ones(E, bool) if masks is None else masks[v]) for v in range(B)]
            bt.append(1e3 * (time.perf_counter() - t0))
        bms = statistics.median(bt)
        put(f"{tag}: {N} poses, {E} edges, {B} variant(s)  solve_dev event {med:10.3f} ms (min {least:10.3f}; host {host:10.3f} ms)  outer iterations {min(its)} .. {max(its)}, "
            f"PCG iterations {pcg}, per PCG iteration {1e3 * med / max(pcg, 1):8.2f} us  baseline {bms:10.3f} ms  baseline / event {bms / med:8.3f}x")
        st = np.bincount(rep["status"], minlength=6)
        put(f"{tag}: statuses (converged, iterations, stalled, singular, unanchored, flipped) {[int(x) for x in st]}; variant 0 cost {float(rep['cost'][0]):.6g} after {its[0]} iterations, "
            f"baseline {base[0][0]:.6g} after {base[0][1]} (status {base[0][2]})")
        return out["o"], rep

    for n in SIZES:
        run(f"loop {n}", scene(n), None)
    G = scene(LOO_SIZE)
    clo = np.arange(G["n_odometry"], len(G["ij"]))
    rows = np.ones((1 + len(clo), len(G["ij"])), bool)
    rows[1 + np.arange(len(clo)), clo] = False
    o, rep = run(f"leave-one-out {LOO_SIZE}", G, rows)
    cost = o["edge_cost"].cpu().numpy()
    loo = cost[1 + np.arange(len(clo)), clo]
    put(f"leave-one-out {LOO_SIZE}: the closures read {loo.min():.4g} .. {loo.max():.4g} (median {np.median(loo):.4g}) under the solutions without them, "
        f"{cost[0, clo].min():.4g} .. {cost[0, clo].max():.4g} under the solution with every edge; report bytes per variant {REPORT_DTYPE.itemsize}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
