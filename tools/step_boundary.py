"""Development aid: the boundary between two C2 step launches, from device wall-clock stamps.

    (build the library with -DAGP_STEP_TRACE)
    python tools/step_boundary.py run  DUMP [--steps N] [--warmup W]    C2-shaped training with AGP_STEP_TRACE=DUMP
    python tools/step_boundary.py table DUMP [DUMP2 ...]                  the stamp table (agp_chol.h, STRACE_*)

`run` trains the bench's C2 model (bench.make_data / bench.build_model, look-ahead on, as bench.py does) and destroys the context,
which writes the dump.  `table` averages the last launches of each dump; every time is in us relative to the end of the chain's
last tile elimination, factor(nt - 1), of the same launch ("next" rows: of the launch before).  Below it, per block column of the
chain: how long the tile elimination and the glue behind it took (the glue split into X_k out + substitution | S = D - L L' up to its
signal | entry of the next elimination, where the library has the STRACE_GLUE stamps) and which way the next column's two feeder tiles came in (prefetched
under the elimination, or late because the look failed / because a sentinel was seen).  Last, the two feeder tiles of block columns
2 .. 6 against the look that wants them: when their workgroup started, finished its product, took the eta2 step and parked.  Between the two, where the library has the STRACE_SUBST stamps: what happens inside "X_k out + substitution"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XPUB, EXT, FILL0, FILL1, WG0, WG1, SAFE0, SAFE1 = 600, 1100, 1400, 1500, 2048, 4096, 6144, 6400
ELIM0, PATH = 528, 560  # per block column k: factor(k) starts ; the path word of column k + 1's feed (PRO_TS, agp_chol.h)
LOOK, NEAR = 608, 640   # the look under factor(k) ; the near-diagonal tiles of block columns 2 .. 6 (STRACE_LOOK, STRACE_NEAR)
SUBST = 1600            # inside the substitution: + 128 w + 16 q + k, waves 0 and 4 (STRACE_SUBST)
GLUE = 1040             # the glue of column k: + k substitution done (S = D - L L' starts), + 16 + k S signalled (STRACE_GLUE)


def run(dump, steps, warm):
    import ctypes as C

    import torch

    sys.path.insert(0, ROOT)
    os.environ["AGP_STEP_TRACE"] = os.path.abspath(dump)
    import bench
    import agp_amd as AGP
    from agp_amd import capi
    from agp_amd import parallel as P

    L = capi.lib()
    dev = torch.device("cuda", 0)
    cfg = dict(bench.CONFIGS["c2"])
    N, m, B = cfg["N"], cfg["m"], cfg["B"]
    X, yh, ell = bench.make_data(cfg, 1234, dev)
    rng = np.random.default_rng(4321)
    Z = X[torch.as_tensor(rng.permutation(N)[:m], device=dev)].cpu().numpy().astype(np.float64)
    total = steps + warm
    idx_all = torch.as_tensor(np.stack([rng.choice(N, B, replace=False) for _ in range(total)]).astype(np.int64), device=dev)
    model = bench.build_model(AGP, cfg, ell, Z, B, 0, 1, 0, "batch")
    model.inference.rho = N / B
    eng = P.HipEngine(model, B).bind_data(X, yh)
    h = eng.h
    xp, yp, ld = C.c_void_p(eng._X.data_ptr()), C.c_void_p(eng._y.data_ptr()), eng._X.stride(0)
    for i in range(total):
        st = L.agp_svgp_cavi_step(h, xp, ld, yp, C.c_void_p(idx_all[i].data_ptr()), B, N / B)
        if st != 0:
            capi.check(model._ctx, st)
        if i + 1 < total:
            L.agp_svgp_prefetch(h, xp, ld, C.c_void_p(idx_all[i + 1].data_ptr()), B)
    model._chk(L.agp_svgp_check_status(h))
    fb = C.c_int64(0)
    model._chk(L.agp_ctx_task_graph_fallbacks(model._ctx, C.byref(fb)))
    torch.cuda.synchronize()
    print(f"[step_boundary] {total} steps, task_graph_fallbacks {fb.value}", flush=True)
    capi.lib().agp_svgp_destroy(model._h)
    model._h = None
    capi.lib().agp_ctx_destroy(model._ctx)
    model._ctx = None


def load(dump):
    with open(dump, "rb") as f:
        n, slots = np.fromfile(f, dtype=np.int64, count=2)
        r = np.fromfile(f, dtype=np.uint64, count=int(n * slots)).reshape(int(n), int(slots)).astype(np.float64)
    r[r == 0] = np.nan
    return r


PATHS = {1: "prefetched", 2: "late: look failed", 3: "late: sentinel in T"}


def columns(cur, nt):
    """per block column k: the tile elimination factor(k) (ELIM0 + k -> 512 + k), the glue behind it (512 + k -> ELIM0 + k + 1: X_k
    out, the substitution, S = D - L L') and how the side job that ran under factor(k) brought in the tiles of column k + 1
    (PATH + k; the last column has none).  Stamps of libraries built before these slots existed read as missing."""
    e0, e1, path = cur[:, ELIM0:ELIM0 + nt], cur[:, 512:512 + nt], cur[:, PATH:PATH + nt]
    if not np.isfinite(e0).any():
        return ["  (no per-column elimination stamps in this dump)"]

    def med(x):
        x = x[np.isfinite(x)]
        return float(np.median(x)) if x.size else float("nan")

    g0, g1 = cur[:, GLUE:GLUE + nt], cur[:, GLUE + 16:GLUE + 16 + nt]
    parts = np.isfinite(g0).any()  # (the glue's own stamps: X_k out + substitution | S = D - L L' up to its signal | entry of factor(k + 1))
    out = ["  per block column: elimination us | glue us" + (" = substitution | product | entry" if parts else "") +
           " | path of the next column's feed (share of launches; median path first)"]
    sums = np.zeros(3)
    for k in range(nt):
        el = med((e1[:, k] - e0[:, k]) * 0.01)
        gl = med((e0[:, k + 1] - e1[:, k]) * 0.01) if k + 1 < nt else float("nan")
        if parts and k + 1 < nt:
            p3 = [med((g0[:, k] - e1[:, k]) * 0.01), med((g1[:, k] - g0[:, k]) * 0.01), med((e0[:, k + 1] - g1[:, k]) * 0.01)]
            sums += p3
            gl = f"{gl:6.2f} = {p3[0]:5.2f} | {p3[1]:5.2f} | {p3[2]:5.2f}"
            gl, glf = float("nan"), gl
        else:
            glf = None
        pk = path[:, k][np.isfinite(path[:, k])].astype(int)
        if pk.size:
            order = sorted(PATHS, key=lambda c: (c != int(np.median(pk)), c))
            what = "  ".join(f"{PATHS[c]} {np.mean(pk == c):4.0%}" for c in order if np.any(pk == c))
        else:
            what = "-"
        out.append(f"    k = {k:2d}  {el:6.2f}  {glf if glf else format(gl, '6.2f')}  {what}")
    if parts:
        out.append(f"  glue, mean over k = 0..{nt - 2}: substitution {sums[0] / (nt - 1):5.2f}   product {sums[1] / (nt - 1):5.2f}   "
                   f"entry {sums[2] / (nt - 1):5.2f}")
    pre = np.array([np.nanmedian(path[:, k]) == 1 for k in range(nt - 1)])
    el = np.array([med((e1[:, k] - e0[:, k]) * 0.01) for k in range(nt)])
    if pre.any():
        out.append(f"  eliminations: prefetched columns (median path) {np.mean(el[:nt - 1][pre]):6.2f}   others "
                   f"{np.mean(el[:nt - 1][~pre]) if (~pre).any() else float('nan'):6.2f}   column {nt - 1} (no side job) {el[nt - 1]:6.2f}")
    return out


SUBST_POINTS = ("X_k read from LDS", "X_k stores issued", "stage 1: MFMAs of L1 = T1 X11'", "after_first (X_k signalled)",
                "L1 stored + barrier", "stage 2: U = T2 - L1 L21', stored + barrier", "stage 3: L2 = U X22', stores issued", "store_d")


def substitution(cur, nt):
    """inside "X_k out + substitution" (512 + k -> GLUE + k): the stamps of wave 0 (short tiles of the triangular stages) and wave 4
    (long tiles; one of the four waves that run store_d), STRACE_SUBST + 128 w + 16 q + k.  Per point the median time since the
    point before it, averaged over the block columns, and the running sum.  The first interval starts at factor(k) done (stamped by
    wave 0 for both), the last one ends at the barrier in front of S = D - L L' (GLUE + k, wave 0)."""
    if not np.isfinite(cur[:, SUBST:SUBST + 256]).any():
        return ["  (no substitution stamps in this dump)"]

    def med(x):
        x = x[np.isfinite(x)]
        return float(np.median(x)) if x.size else float("nan")

    out = ["  inside X_k out + substitution, us since the point before, mean over k = 0.." + str(nt - 2) +
           " of the medians (running sum): wave 0 (short tiles) | wave 4 (long tiles, store_d)"]
    run = np.zeros(2)
    prev = [cur[:, 512:512 + nt - 1]] * 2
    for q, what in enumerate(SUBST_POINTS + ("barrier in front of S = D - L L'",)):
        cells = []
        for w in range(2):
            at = cur[:, GLUE:GLUE + nt - 1] if q == len(SUBST_POINTS) else cur[:, SUBST + 128 * w + 16 * q:SUBST + 128 * w + 16 * q + nt - 1]
            if not np.isfinite(at).any():  # (a point this library does not stamp: its time goes to the next one)
                cells.append(f"{'-':>5} ({run[w]:5.2f})")
                continue
            d = np.mean([med((at[:, k] - prev[w][:, k]) * 0.01) for k in range(nt - 1)])
            run[w] += d
            prev[w] = at
            cells.append(f"{d:5.2f} ({run[w]:5.2f})")
        out.append(f"    {what:<44} {cells[0]} | {cells[1]}")
    return out


def tile_slot(R, c):
    """first stamp of matrix tile (R, c): PRO_TS's old region for R, c < 4, STRACE_NEAR for the near tiles of block columns 2 .. 6"""
    if R < 4 and c < 4:
        return 64 + 8 * (4 * R + c)
    if 2 <= c <= 6 and 0 <= R - c < 4:
        return NEAR + 8 * (4 * (c - 2) + (R - c))
    return None


def feeders(cur, nt):
    """the two feeder tiles of block column k + 1, (k + 1, k) and (k + 1, k + 1), against the look that needs them (the side job
    under factor(k)): median us relative to that look, negative = before it.  start: the workgroup reaches its prologue; product: own
    k-slice done; helpers: all partial tiles signalled; stepped: partials added and the eta2 step taken; parked: updates of the
    earlier columns applied, tile parked and signalled.  Late: share of launches in which the tile was parked after the look."""
    look = cur[:, LOOK:LOOK + nt]
    if not np.isfinite(look).any():
        return ["  (no look stamps in this dump)"]

    def med(x):
        x = x[np.isfinite(x)]
        return float(np.median(x)) if x.size else float("nan")

    out = ["  feeders against the look under factor(k), us (negative: before the look):",
           "    k  tile      start  product  helpers  stepped   parked   late | factor(k) start  X_(k-1) out -> look"]
    for k in range(1, min(nt - 1, 6)):
        for R, c in ((k + 1, k), (k + 1, k + 1)):
            s = tile_slot(R, c)
            if s is None:
                continue
            rel = lambda q: med((cur[:, s + q] - look[:, k]) * 0.01)
            late = np.nanmean((cur[:, s + 5] > look[:, k])[np.isfinite(cur[:, s + 5]) & np.isfinite(look[:, k])])
            out.append(f"   {k:2d}  ({R},{c})  {rel(0):8.2f} {rel(1):8.2f} {rel(2):8.2f} {rel(4):8.2f} {rel(5):8.2f}  {late:5.0%} | "
                       f"{med((cur[:, ELIM0 + k] - look[:, k]) * 0.01):8.2f}         {med((cur[:, 512 + k - 1] - look[:, k]) * 0.01):8.2f}")
    return out


def table(dumps, last=200, nt=16, ne=17):
    rows = []
    for dump in dumps:
        r = load(dump)[-last - 1:]
        cur, prev = r[1:], r[:-1]
        f_end = cur[:, 512 + nt - 1]  # factor(nt - 1) done
        us = lambda a: (a - f_end[:, None] if a.ndim == 2 else a - f_end) * 0.01  # 100 MHz ticks -> us
        pf_end = prev[:, 512 + nt - 1]
        pus = lambda a: (a - pf_end[:, None] if a.ndim == 2 else a - pf_end) * 0.01

        def med(x):
            x = x[np.isfinite(x)]
            return float(np.median(x)) if x.size else float("nan")

        out = [f"== {os.path.basename(dump)}: {len(cur)} launches; median us relative to factor({nt - 1}) done =="]
        out.append(f"  launch t:   first workgroup start           {med(np.nanmin(us(cur[:, WG0:WG1]), axis=1)):8.2f}")
        out.append(f"              chain start (tile 0,0)          {med(us(cur[:, 0])):8.2f}")
        out.append(f"              tile (0,0) ready (eta2 step)    {med(us(cur[:, 4])):8.2f}")
        out.append(f"              factor(0) done                  {med(us(cur[:, 512])):8.2f}")
        out.append(f"              factor({nt - 1}) done                 {0.0:8.2f}")
        out.append(f"              X_{nt - 1} published                 {med(us(cur[:, XPUB])):8.2f}")
        ext = lambda q: us(cur[:, EXT + 4 * np.arange(ne) + q])
        for q, what in enumerate(("X seen", "W stored + signalled", "v tile read (epilogue)", "rows finished")):
            e = ext(q)
            if q >= 2:
                e = e[:, :ne - 1]  # (the [eta1' ; 0] row has no epilogue)
            out.append(f"              ext rows (R,{nt - 1}) {what:<23} first {med(np.nanmin(e, axis=1)):8.2f}  last "
                       f"{med(np.nanmax(e, axis=1)):8.2f}")
        out.append(f"              refill workgroups start / end   {med(np.nanmin(us(cur[:, FILL0:FILL0 + 64]), axis=1)):8.2f} "
                   f"{med(np.nanmax(us(cur[:, FILL1:FILL1 + 64]), axis=1)):8.2f}")
        out.append(f"              last workgroup exit             {med(np.nanmax(us(cur[:, WG1:SAFE0]), axis=1)):8.2f}")
        out.append(f"  behind it:  k_safe_rowstats start / end    {med(np.nanmin(us(cur[:, SAFE0:SAFE1]), axis=1)):8.2f} "
                   f"{med(np.nanmax(us(cur[:, SAFE1:SAFE1 + 256]), axis=1)):8.2f}")
        out.append(f"  launch t+1: first workgroup start           {med(np.nanmin(pus(cur[:, WG0:WG1]), axis=1)):8.2f}")
        out.append(f"              tile (0,0) ready (eta2 step)    {med(pus(cur[:, 4])):8.2f}")
        out.append(f"              factor(0) done                  {med(pus(cur[:, 512])):8.2f}")
        f = cur[:, 512:512 + nt]  # the chain, block column by block column
        d = np.array([med(c) for c in (np.diff(f, axis=1) * 0.01).T])
        out.append(f"== {os.path.basename(dump)}: {len(cur)} launches; median us between the ends of consecutive tile eliminations ==")
        out.append(f"  factor(k) - factor(k-1), k = 1..{nt - 1}: " + " ".join(f"{x:6.2f}" for x in d))
        out.append(f"  mean over k {np.mean(d):6.3f}   factor({nt - 1}) - factor(0) {med(f[:, nt - 1] - f[:, 0]) * 0.01:8.2f}")
        out.append(f"  chain start -> factor(0) done {med(f[:, 0] - cur[:, 0]) * 0.01:8.2f}")
        out += columns(cur, nt)
        out += substitution(cur, nt)
        out += feeders(cur, nt)
        rows += out
    return "\n".join(rows)


if __name__ == "__main__":
    if sys.argv[1] == "run":
        a = sys.argv[2:]
        steps = int(a[a.index("--steps") + 1]) if "--steps" in a else 200
        warm = int(a[a.index("--warmup") + 1]) if "--warmup" in a else 20
        run(a[0], steps, warm)
    else:
        print(table(sys.argv[2:]))
