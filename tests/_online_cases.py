"""Inputs of the streaming-model edge tests, shared by tests/test_online_cases_host.py (which proves on the CPU, with the oracle
alone, that the inputs have the properties the device tests rely on) and tests/test_gpu_online_edges.py (which compares the device
with the oracle on exactly these inputs).  No GPU import.

What the cases reach: every matrix of the streaming prior is rectangular, `map x mp` or `map x map` with map = rup64(ma) the padded
number of OLD inducing points and mp = rup64(m) that of the new ones (set_online_prior, online_refresh, extra_kl and the online
branch of hypergrad() in csrc/agp_capi.hip).  The cases make map != mp in both directions, put both above one tile, and make the old
set NOT a subset of the new one, so that K~_a = K_a - kappa_a K_ab' and the terms it multiplies do not vanish.

Two generators:

* `lattice_stream`: data for the real OIPS rule.  Batch b holds counts[b] not yet seen sites of an integer lattice (spacing 1) and
  Bs[b] - counts[b] "followers": a site seen before plus uniform noise of at most FOLLOW per coordinate.  Under the kernel
  VARIANCE * SqExponential o ScaleTransform(SCALE) a new site's largest kernel value with Z is 1.2 exp(-1.6^2 / 2) = 0.334 and a
  follower's at least 1.2 exp(-D (1.6 * 0.03)^2 / 2) >= 1.195 (D <= 3) against the threshold RHO = 0.7: the selection is the same in
  fp64 and fp32, on the device and on the host, and m after batch b is exactly cumsum(counts)[b].
* `scripted_sets` with the rule `Scripted`: prescribed inducing sets, each built from the previous one minus some points, with
  some survivors moved, plus fresh lattice sites.  `Scripted` has the oracle's Zalg interface; the device side installs it with
  `device_rule` in place of agp_amd.online._oips_update.
"""
import functools

import numpy as np

VARIANCE, SCALE, RHO, FOLLOW = 1.2, 1.6, 0.7, 0.03
ARD2 = (1.6, 1.3)  # ARDTransform of the scripted cases at D = 2
TILE = 64

# the growth case: m = 40, 63, 64, 65, 65, 128, 130 -> (map, mp) = (64, 64) x3, (64, 128), (128, 128), (128, 128), (128, 192);
# B below m, B off the tile grid, one batch that adds no point
GROWTH_COUNTS = (40, 23, 1, 1, 0, 63, 2)
GROWTH_BS = (60, 64, 65, 50, 37, 130, 129)
# the scripted sequences: (63, 65, 130, 70, 60) has ma > m twice, 130 -> 70 (map = 192 > mp = 128) and 70 -> 60 (128 > 64)
SEQ_A = (63, 65, 130, 70, 60)
SEQ_B = (64, 64, 128, 129)
DROP, MOVE, SHIFT = 3, 5, 0.3
NEAR = 24
B_SCRIPTED, ITERS_SCRIPTED, ITERS_GROWTH = 130, 5, 3


def rup64(n):
    return (n + TILE - 1) // TILE * TILE


def _sites(D, total, rng):
    """`total` distinct sites of the smallest cube {0 .. side-1}^D that holds them, in random order"""
    side = 1
    while side ** D < total:
        side += 1
    all_sites = np.array(list(np.ndindex(*([side] * D))), dtype=np.float64)
    return all_sites[rng.permutation(len(all_sites))[:total]], side


def lattice_stream(D, counts, Bs, seed):
    """list of (Bs[b], D) batches (see the module docstring).  A follower always comes after the site it follows, so the first point of
    the stream is a site and no follower is ever accepted."""
    rng = np.random.default_rng(seed)
    sites, _ = _sites(D, int(np.sum(counts)), rng)
    out, seen = [], 0
    for c, B in zip(counts, Bs):
        assert 0 <= c <= B and (seen + c > 0)
        batch = [("s", seen + i) for i in range(c)]
        for _ in range(B - c):
            parent = int(rng.integers(seen + c))
            lo = 1 + batch.index(("s", parent)) if parent >= seen else 0
            batch.insert(int(rng.integers(lo, len(batch) + 1)), ("f", parent))
        X = np.array([sites[i] + (0.0 if kind == "s" else rng.uniform(-FOLLOW, FOLLOW, D)) for kind, i in batch])
        out.append(X)
        seen += c
    return out


def scripted_sets(sizes, drop=DROP, move=MOVE, seed=0, D=2, spacing=1.0):
    """list of (sizes[b], D) inducing sets.  Set b+1 keeps min(n_b, sizes[b+1]) - drop points of set b (so at least `drop` leave and at
    least `drop` fresh sites arrive, whether the set grows or shrinks), puts `move` of the kept ones at a new place within SHIFT of
    their own lattice site, and fills up with lattice sites never used before.  Returns (sets, box): box is the side of the cube."""
    rng = np.random.default_rng(seed)
    fresh_total = sizes[0] + sum(sizes[b + 1] - (min(sizes[b], sizes[b + 1]) - drop) for b in range(len(sizes) - 1))
    sites, side = _sites(D, fresh_total, rng)
    home = list(range(sizes[0]))            # lattice site of every point of the current set
    pos = [sites[i].copy() for i in home]
    used = sizes[0]
    sets = [np.array(pos) * spacing]
    for n in sizes[1:]:
        keep = np.sort(rng.permutation(len(home))[:min(len(home), n) - drop])
        home, pos = [home[i] for i in keep], [pos[i] for i in keep]
        for i in rng.permutation(len(home))[:move]:
            pos[i] = sites[home[i]] + rng.uniform(-SHIFT, SHIFT, D)
        add = n - len(home)
        home += list(range(used, used + add))
        pos += [sites[i].copy() for i in range(used, used + add)]
        used += add
        sets.append(np.array(pos) * spacing)
    assert used == fresh_total
    return sets, side * spacing


class Scripted:
    """A Zalg (oracle interface: init, update, remove_point) that returns prescribed sets: sets[l][b] for latent l at batch b.  Both
    models ask once per latent and batch, latents in order."""

    rho_remove = 1.0  # (the device's train_online reads it: no removal step)

    def __init__(self, sets):
        self.sets, self.calls = sets, 0

    def _next(self):
        l, b = self.calls % len(self.sets), self.calls // len(self.sets)
        self.calls += 1
        return np.array(self.sets[l][b], dtype=np.float64)

    def init(self, X, kernel):
        return self._next()

    def update(self, Z, X, kernel):
        return self._next()

    def remove_point(self, rng, Z, Kmat):
        return Z


def device_rule(alg, host, kernel, Z, X):
    """stands in for agp_amd.online._oips_update when the model's Zalg is a Scripted"""
    return alg.update(Z, X, kernel)


def _latent_f(X, box):
    u = X / box
    return np.sin(5.0 * u[:, 0]) + 0.5 * np.cos(4.0 * u[:, -1] + u.sum(axis=1) / X.shape[1])


def stream_labels(likname, Xs, box, seed):
    """targets of every batch (tests/_liks.py generators; every batch of a multi-class stream holds all three classes)"""
    from _liks import labels

    rng = np.random.default_rng(seed + 1000)
    return [labels(likname, _latent_f(X, box), X, rng) for X in Xs]


@functools.lru_cache(maxsize=None)
def growth_case(D, likname="logistic", seed=0):
    Xs = lattice_stream(D, GROWTH_COUNTS, GROWTH_BS, seed + D)
    box = float(np.max(np.concatenate(Xs))) + 1.0
    rng = np.random.default_rng(seed + 77)
    return dict(name=f"growth-D{D}-{likname}", D=D, lik=likname, Xs=Xs, ys=stream_labels(likname, Xs, box, seed), box=box,
                kind="sqexponential", scale=SCALE, iters=ITERS_GROWTH, m_seq=tuple(int(v) for v in np.cumsum(GROWTH_COUNTS)),
                Xt=rng.uniform(-0.5, box - 0.5, (70, D)))


def growth_sets(D, seed=0):
    """the sets OIPS picks on the growth stream: the new sites in their order of arrival"""
    Xs = lattice_stream(D, GROWTH_COUNTS, GROWTH_BS, seed + D)
    Z, sets = np.zeros((0, D)), []
    for X in Xs:
        new = X[np.all(X == np.round(X), axis=1)]
        Z = np.concatenate([Z, new])
        sets.append(Z.copy())
    return sets


# D = 9: ARD scales between 1.5 and 2.0, so neighbouring sites keep a kernel value of at most 1.2 exp(-1.5^2 / 2) = 0.39
ARD9 = tuple(1.5 + 0.5 * np.linspace(0.0, 1.0, 9) ** 2)


@functools.lru_cache(maxsize=None)
def scripted_case(seq, likname="logistic", D=2, kind="matern52", seed=0, B=B_SCRIPTED):
    sizes = {"A": SEQ_A, "B": SEQ_B}[seq]
    sets, box = scripted_sets(sizes, seed=seed, D=D)
    rng = np.random.default_rng(seed + 31)
    # uniform over the box, but NEAR of every batch's points sit around the last DROP points of that batch's set: what the model learns
    # about them comes from this batch alone, so a prior that loses them at the next hand-over (index >= 64) is visibly another one
    Xs = []
    for Z in sets:
        near = np.repeat(Z[-DROP:], NEAR // DROP, axis=0) + rng.uniform(-0.4, 0.4, (NEAR // DROP * DROP, D))
        X = np.concatenate([rng.uniform(-0.5, box - 0.5, (B - len(near), D)), near])
        Xs.append(X[rng.permutation(B)])
    return dict(name=f"scripted-{seq}-D{D}-{kind}-{likname}", D=D, lik=likname, Xs=Xs, ys=stream_labels(likname, Xs, box, seed),
                box=box, kind=kind, scale=np.array(ARD2 if D == 2 else ARD9[:D]), iters=ITERS_SCRIPTED, m_seq=sizes, sets=sets,
                Xt=rng.uniform(-0.5, box - 0.5, (70, D)))


def oracle_kernel(R, c):
    return R.Kernel(c["kind"], c["scale"], VARIANCE)


def device_kernel(AGP, c):
    base = {"sqexponential": AGP.SqExponentialKernel, "matern52": AGP.Matern52Kernel}[c["kind"]]()
    tr = AGP.ARDTransform(np.asarray(c["scale"])) if np.ndim(c["scale"]) else AGP.ScaleTransform(c["scale"])
    return VARIANCE * (base @ tr)


def combos(c, B=None):
    """(ma, m, map, mp, B, D) of every hand-over of a case"""
    ms = c["m_seq"]
    return [(ms[b - 1], ms[b], rup64(ms[b - 1]), rup64(ms[b]), len(c["Xs"][b]) if B is None else B, c["D"])
            for b in range(1, len(ms))]
