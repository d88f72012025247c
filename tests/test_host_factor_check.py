"""The element-scaled check of the factor gradients (problems.factor_check) on the CPU alone.

(a) Two twins of a correct kernel pass with at least 10x margin on a representative subset of the problems the GPU files
    run: the f32 build of the oracle (sequential f32 sums: the exact kernel's roundings), and a numpy twin of the split
    kernels' gradient products -- G = g sigma delta rounded to f32, both operands split into bf16 hi and mid, the sum
    hi hi + hi mid + mid hi taken in fp64.  (The C oracle has no squared-hinge columns: on those problems the first twin is
    numpy's f32 product of the f32-rounded operands.)
(b) The check fails, with a worst ratio of at least 10, when the problem is mutated the way a kernel bug would corrupt a
    gradient: a 32 x 32 tile of D that contributes nothing, a column run with its neighbour's sigma, mu and weight, a row
    in the neighbouring batch, a noise-range boundary off by one column, the last batch of a view sent to the identity
    slot, one observed entry dropped.
(c) What rel_err <= GRAD_TOL does not see: on the 1025 x 300 mixed problem at least half of the dropped tiles pass it.
(d) A gradient built to cancel (M = 31, N = 1) passes with the f32 oracle, where rel_err does not.
(e) layer_scales returns, bit for bit, what it returned before its per-entry part moved to entry_scales.
(f) The failure message names the element, its column's noise kind and views, and the tile that went missing.

Measured (FACTOR_TWIN / FACTOR_MUTANT lines of this file): f32 twin <= 0.0067, split twin <= 0.081; smallest mutant ratios:
tile 31.7, column 78, row 218, boundary 1247, identity slot 429, dropped entry 10.2 (28 % to 81 % of the observed entries
qualify); 16 of 20 dropped tiles of the 1025 x 300 problem pass rel_err <= GRAD_TOL.
"""
import copy
import functools

import numpy as np
import pytest

import batch_cases as bc
import hinge_ref as hr
from problems import (FACTOR_TAU, LAYER_TAU, entry_scales, factor_check, factor_scales, factor_worst, layer_scales,
                      make_problem, rel_err, to_oracle)
from test_gpu_edges import data_kw, expected_family, panel_shapes, range_problem, range_seed
from test_gpu_parity import CASES, GRAD_TOL
from test_gpu_split_bf16 import bf16_round

BOTH = dict(update_X=True, update_Y=True)
GENERAL = dict(bernoulli_frac=0.2, poisson_frac=0.1, n_views=2, batch_views=2, n_batches=6, col_params=True, weights=True,
               nan_frac=0.05, scale=0.4)


def test_tau_is_the_layer_checks():
    assert FACTOR_TAU == LAYER_TAU == 2e-5


# ---- the problems ----------------------------------------------------------------------------------------------------
def _k_edge(K, s):
    M, N = panel_shapes(expected_family(K, "f32", True)[1])[s]
    return make_problem(M=M, N=N, K=K, seed=K * 7 + M + N, **data_kw(K))


def _general(K):
    return make_problem(M=expected_family(K, "f32", True, batch=True)[1] + 1, N=161, K=K, seed=K + 5, **GENERAL)


def _bf16_stored(K):
    p = make_problem(M=expected_family(K, "bf16x3", True)[1] + 33, N=95, K=K, seed=K + 9, **data_kw(K))
    p["D"] = np.asfortranarray(bf16_round(p["D"]))
    return p


def _ranges(K, prec, mixed):
    return range_problem(expected_family(K, prec, True, batch=mixed)[1] + 33, 161, K, mixed, range_seed(K, mixed))


SHAPES = {f"k{K}-shape{s}": functools.partial(_k_edge, K, s) for K in (1, 32, 33, 64, 65, 96, 97, 128) for s in range(4)}
SHAPES.update({f"general-k{K}": functools.partial(_general, K) for K in (32, 33, 64, 65, 96, 97, 128)})
SHAPES.update({f"bf16-stored-k{K}": functools.partial(_bf16_stored, K) for K in (33, 64, 97, 128)})
SHAPES.update({f"parity-{name}": functools.partial(make_problem, seed=11, **kw) for name, kw in CASES.items()})
_seen = set()
for _id, _fn, _path, _BM in bc.all_cases():
    _key = (_fn.func, _fn.args)
    if _key not in _seen:                        # one problem runs on several paths
        _seen.add(_key)
        SHAPES[f"batch-{_id}"] = _fn
SHAPES.update({f"hinge-{name}": (lambda p=p: p) for name, p in hr.all_problems()})
SHAPES.update({f"ranges-k{K}-{prec}-{'mixed' if mixed else 'plain'}": functools.partial(_ranges, K, prec, mixed)
               for K in (32, 64, 96, 128) for prec in ("f32", "bf16x3") for mixed in (True, False)})


def data_oracle(p, precision=64):
    """Loss and data gradients (the regularizers left out) of the C oracle."""
    m = to_oracle(p, precision)
    m.m.n_xreg = 0
    m.m.n_yreg = 0
    return m.loss_and_grads(**BOTH)[1]


def split(a):
    """bf16 hi and mid of an f32 array, as fp64."""
    a = np.asarray(a, np.float32)
    hi = bf16_round(a)
    mid = bf16_round(a - hi)
    return hi.astype(np.float64), mid.astype(np.float64)


def twins(p):
    """(want, f32 twin, split twin): gX and gY in fp64, from an f32 evaluation, and from the three-product bf16 split."""
    X, Y = np.asarray(p["X"], np.float32), np.asarray(p["Y"], np.float32)
    (Xh, Xm), (Yh, Ym) = split(X), split(Y)
    M, N = p["D"].shape
    sp = dict(X=np.zeros(X.shape), Y=np.zeros(Y.shape))
    f32 = dict(X=np.zeros(X.shape, np.float32), Y=np.zeros(Y.shape, np.float32))
    cols = max(32, (1 << 22) // M)                      # blocks of columns: the tall problems stay cheap
    for c0 in range(0, N, cols):
        c1 = min(N, c0 + cols)
        e = entry_scales(p, c0, c1)
        G = (e["g"] * e["sd"]).astype(np.float32)
        Gh, Gm = split(G)
        sp["X"] += Yh[:, c0:c1] @ Gh.T + Yh[:, c0:c1] @ Gm.T + Ym[:, c0:c1] @ Gh.T
        sp["Y"][:, c0:c1] = Xh @ Gh + Xh @ Gm + Xm @ Gh
        f32["X"] += Y[:, c0:c1] @ G.T
        f32["Y"][:, c0:c1] = X @ G
    if p.get("noise_thr"):
        want = hr.reference_of(p)
    else:
        want, f32 = data_oracle(p), data_oracle(p, 32)
    return want, f32, sp


@pytest.mark.parametrize("name", list(SHAPES))
def test_twins_pass_with_margin(name):
    p = SHAPES[name]()
    want, f32, sp = twins(p)
    assert np.isfinite(want["X"]).all() and np.isfinite(want["Y"]).all()
    s = factor_scales(p)
    w32, wsp = factor_check(p, f32, want, scales=s), factor_check(p, sp, want, scales=s)
    print(f"FACTOR_TWIN {name} f32 X={w32['X']:.4f} Y={w32['Y']:.4f} split X={wsp['X']:.4f} Y={wsp['Y']:.4f}")
    assert max(w32.values()) <= 0.1, w32
    assert max(wsp.values()) <= 0.1, wsp


# ---- mutants ---------------------------------------------------------------------------------------------------------
MUTATED = {
    "mixed-1025x300-k64": functools.partial(make_problem, M=1025, N=300, K=64, seed=71, **GENERAL),
    "mixed-129x161-k128": functools.partial(make_problem, M=129, N=161, K=128, seed=133, **GENERAL),
    "mixed-257x161-k64": functools.partial(make_problem, M=257, N=161, K=64, seed=69, **GENERAL),
    "ranges-k64-f32-mixed": functools.partial(_ranges, 64, "f32", True),
    "ranges-k128-bf16x3-plain": functools.partial(_ranges, 128, "bf16x3", False),
}
DROPPED = dict(MUTATED)
DROPPED["mixed-257x161-k32"] = functools.partial(make_problem, M=257, N=161, K=32, seed=37, **GENERAL)


@functools.lru_cache(maxsize=None)
def base(name):
    """(problem, fp64 data gradients, factor scales) of a mutated problem, once."""
    p = DROPPED[name]()
    return p, data_oracle(p), factor_scales(p)


def ratio(name, q):
    """Worst ratio of the mutant q's fp64 gradients against the original's, at the original's scales."""
    p, want, s = base(name)
    return max(factor_check(p, data_oracle(q), want, scales=s).values())


def drop_tile(p, ti, tj):
    q = copy.deepcopy(p)
    q["D"][32 * ti:32 * ti + 32, 32 * tj:32 * tj + 32] = np.nan
    return q


def tile_draws(p, n, seed):
    rng = np.random.default_rng(seed)
    nt = ((p["M"] + 31) // 32, (p["N"] + 31) // 32)
    return [divmod(int(t), nt[1]) for t in rng.choice(nt[0] * nt[1], size=min(n, nt[0] * nt[1]), replace=False)]


@pytest.mark.parametrize("name", list(MUTATED))
def test_a_tile_that_contributes_nothing_fails(name):
    p = base(name)[0]
    r = [ratio(name, drop_tile(p, ti, tj)) for ti, tj in tile_draws(p, 20, 1)]
    print(f"FACTOR_MUTANT {name} tile min={min(r):.1f}")
    assert min(r) >= 10, r


@pytest.mark.parametrize("name", list(MUTATED))
def test_a_column_with_its_neighbours_parameters_fails(name):
    p = base(name)[0]
    r = []
    for j in np.random.default_rng(2).choice(p["N"] - 1, size=25, replace=False):
        q = copy.deepcopy(p)
        for k in ("logsigma", "mu", "col_weight"):
            q[k][j] = p[k][j + 1]
        r.append(ratio(name, q))
    print(f"FACTOR_MUTANT {name} column min={min(r):.1f}")
    assert min(r) >= 10, r


@pytest.mark.parametrize("name", [n for n in MUTATED if "plain" not in n])
def test_a_row_in_the_neighbouring_batch_fails(name):
    p = base(name)[0]
    rng = np.random.default_rng(3)
    r = []
    for i in rng.choice(p["M"], size=15, replace=False):
        v = int(rng.integers(len(p["batch_views"])))
        q = copy.deepcopy(p)
        bor, nb = q["batch_views"][v]["batch_of_row"], q["batch_views"][v]["logdelta"].shape[0]
        bor[i] = bor[i] + 1 if bor[i] + 1 < nb else bor[i] - 1
        r.append(ratio(name, q))
    print(f"FACTOR_MUTANT {name} row min={min(r):.1f}")
    assert min(r) >= 10, r


@pytest.mark.parametrize("name", [n for n in MUTATED if "plain" not in n])
def test_a_noise_boundary_off_by_one_column_fails(name):
    p = base(name)[0]
    r = []
    for b in range(len(p["noise_ranges"]) - 1):
        for d in (-1, 1):
            q = copy.deepcopy(p)
            (s0, e0), (s1, e1) = p["noise_ranges"][b], p["noise_ranges"][b + 1]
            q["noise_ranges"][b], q["noise_ranges"][b + 1] = (s0, e0 + d), (s1 + d, e1)
            r.append(ratio(name, q))
    print(f"FACTOR_MUTANT {name} boundary min={min(r):.1f}")
    assert len(r) == 4 and min(r) >= 10, r


@pytest.mark.parametrize("name", [n for n in MUTATED if "plain" not in n])
def test_the_last_batch_in_the_identity_slot_fails(name):
    p = base(name)[0]
    r = []
    for v in range(len(p["batch_views"])):
        q = copy.deepcopy(p)
        bor = q["batch_views"][v]["batch_of_row"]
        bor[bor == q["batch_views"][v]["logdelta"].shape[0] - 1] = -1
        r.append(ratio(name, q))
    print(f"FACTOR_MUTANT {name} identity min={min(r):.1f}")
    assert min(r) >= 10, r


@pytest.mark.parametrize("name", list(DROPPED))
def test_a_dropped_entry_fails(name):
    """Entries whose own term exceeds 10 tau scale in some element of gY or gX (the others cannot be seen by any check at
    this tau); the share of the observed entries that qualify is printed, not bounded: it falls with M and N."""
    p, want, s = base(name)
    e = entry_scales(p)
    G = np.abs(e["g"] * e["sd"])
    Xa, Ya = np.abs(np.asarray(p["X"], np.float64)), np.abs(np.asarray(p["Y"], np.float64))
    big = np.zeros(G.shape, bool)
    for k in range(p["K"]):
        big |= G * Xa[k][:, None] > 10 * FACTOR_TAU * s["Y"][k][None, :]
        big |= G * Ya[k][None, :] > 10 * FACTOR_TAU * s["X"][k][:, None]
    obs = np.isfinite(p["D"])
    big &= obs
    i, j = np.nonzero(big)
    r = []
    for n in np.random.default_rng(4).choice(len(i), size=10, replace=False):
        q = copy.deepcopy(p)
        q["D"][i[n], j[n]] = np.nan
        r.append(ratio(name, q))
    print(f"FACTOR_MUTANT {name} entry share={big.sum() / obs.sum():.3f} min={min(r):.1f}")
    assert min(r) >= 10 * (1 - 1e-9), r


def test_rel_err_misses_most_dropped_tiles_of_a_mixed_problem():
    name = "mixed-1025x300-k64"
    p, want, s = base(name)
    passed, r = 0, []
    for ti, tj in tile_draws(p, 20, 5):
        got = data_oracle(drop_tile(p, ti, tj))
        passed += rel_err(got["X"], want["X"]) <= GRAD_TOL and rel_err(got["Y"], want["Y"]) <= GRAD_TOL
        r.append(max(factor_check(p, got, want, scales=s).values()))
    print(f"FACTOR_MUTANT {name} tiles passing rel_err {passed}/20; factor_check min={min(r):.1f}")
    assert passed >= 10, passed
    assert min(r) > 1, r


def test_the_failure_message_names_the_element_its_column_and_the_tile():
    name = "mixed-257x161-k64"
    p, want, s = base(name)
    got = data_oracle(drop_tile(p, 2, 3))                   # rows 64..95 x columns 96..127: Gaussian columns of view 1
    msg = factor_worst(p, got, want, scales=s).split("\n")
    assert len(msg) == 2 and msg[0].startswith("gX[k=") and msg[1].startswith("gY[k="), msg
    for line in msg:
        assert "tile (row block 2, column block 3)" in line, line
        assert ("masked" if np.isnan(p["D"][64:96, 96:128]).any() else "all-finite") in line, line
    assert "noise normal, view 1, batch view 1" in msg[1], msg[1]
    assert not np.isfinite(factor_check(p, dict(Y=np.full_like(want["Y"], np.nan)), want, scales=s)["Y"])
    assert factor_check(p, dict(X=want["X"]), want, scales=s) == {"X": 0.0}     # only the gradients present


def test_cancelling_sums_pass_with_the_f32_oracle():
    """M = 31, N = 1: D = z + e with e orthogonal to every row of X, so every element of gY cancels to rounding noise.
    rel_err divides by that noise; the element check does not."""
    M, N, K = 31, 1, 4
    p = make_problem(M=M, N=N, K=K, seed=5, col_params=True, weights=True)
    rng = np.random.default_rng(6)
    z = to_oracle(p).forward()[:, 0]
    X = np.asarray(p["X"], np.float64)
    e = rng.standard_normal(M)
    e -= X.T @ np.linalg.lstsq(X.T, e, rcond=None)[0]
    p["D"] = np.asfortranarray((z + 0.3 * e)[:, None].astype(np.float32))
    g64, g32 = data_oracle(p), data_oracle(p, 32)
    s = factor_scales(p)
    assert np.all(np.abs(g64["Y"]) < 1e-5 * s["Y"]), "the problem does not cancel"
    assert rel_err(g32["Y"], g64["Y"]) > GRAD_TOL            # rel_err misfires here
    worst = factor_check(p, g32, g64, scales=s)
    assert max(worst.values()) <= 0.1, worst


# ---- layer_scales is what it was -------------------------------------------------------------------------------------
def layer_scales_before(p, cols=4096):
    """problems.layer_scales as it stood before entry_scales was taken out of it, kept verbatim for the comparison below."""
    X = np.asarray(p["X"], np.float64)
    Y = np.asarray(p["Y"], np.float64)
    D = p["D"]
    M, N = D.shape
    sig_all = np.exp(np.asarray(p["logsigma"], np.float64))
    mu_all = np.asarray(p["mu"], np.float64)
    w_all = np.asarray(p["col_weight"], np.float64)
    kind = np.zeros(N, np.int8)                                   # 0 normal, 1 bernoulli, 2 poisson
    for (s, e), kd in zip(p["noise_ranges"], p["noise_kinds"]):
        kind[s - 1:e] = {"normal": 0, "bernoulli": 1, "poisson": 2}[kd]
    bvs = []
    for bv in p["batch_views"]:
        bor = np.asarray(bv["batch_of_row"])
        nb = np.asarray(bv["logdelta"]).shape[0]
        bvs.append((bv["start1"] - 1, bv["stop1"], bor, bor >= 0, nb, np.exp(np.asarray(bv["logdelta"], np.float64)),
                    np.asarray(bv["theta"], np.float64), (bor[:, None] == np.arange(nb)[None, :]).astype(np.float64)))
    out = dict(mu=np.zeros(N), logsigma=np.zeros(N), theta=[np.zeros((b[4], b[1] - b[0])) for b in bvs],
               logdelta=[np.zeros((b[4], b[1] - b[0])) for b in bvs], g=np.zeros((M, N)), loss=0.0)
    for c0 in range(0, N, cols):
        c1 = min(N, c0 + cols)
        sig, mu, w, kd = sig_all[c0:c1], mu_all[c0:c1], w_all[c0:c1], kind[c0:c1]
        A = X.T @ Y[:, c0:c1]
        Aabs = np.abs(X).T @ np.abs(Y[:, c0:c1])
        dl = np.ones_like(A)
        th = np.zeros_like(A)
        for s, e, bor, has, nb, delta, theta, onehot in bvs:
            a, b = max(s, c0), min(e, c1)
            if a < b:
                dl[np.ix_(has, np.arange(a - c0, b - c0))] = delta[bor[has]][:, a - s:b - s]
                th[np.ix_(has, np.arange(a - c0, b - c0))] = theta[bor[has]][:, a - s:b - s]
        z1 = A * sig[None, :]
        z = z1 * dl + mu[None, :] + th
        link, dlink = z.copy(), np.ones_like(z)
        bern, pois = kd == 1, kd == 2
        sg = 0.5 * (1.0 + np.tanh(0.5 * z[:, bern]))
        link[:, bern], dlink[:, bern] = sg, sg * (1.0 - sg)
        link[:, pois] = dlink[:, pois] = np.exp(z[:, pois])
        Dc = np.asarray(D[:, c0:c1], np.float64)
        obs = np.isfinite(Dc)
        y = np.where(obs, Dc, 0.0)
        g = np.where(obs, w[None, :] * (link - y), 0.0)
        r = sig[None, :] * Aabs * dl + np.abs(mu)[None, :] + np.abs(th)
        sG = np.where(obs, w[None, :] * (np.abs(link) + np.abs(y) + dlink * r), 0.0)
        sQ = np.abs(z1) * sG + np.abs(g) * sig[None, :] * Aabs
        lm = np.where(kd[None, :] == 0, 0.5 * (z - y) ** 2,
                      np.where(kd[None, :] == 1, np.logaddexp(0.0, z), np.exp(np.minimum(z, 700.0))) + np.abs(y * z))
        out["loss"] += float(np.sum(np.where(obs, w[None, :] * lm, 0.0)))
        out["g"][:, c0:c1] = g
        out["mu"][c0:c1] = sG.sum(0)
        out["logsigma"][c0:c1] = sig * (dl * sG).sum(0)
        for v, (s, e, bor, has, nb, delta, theta, onehot) in enumerate(bvs):   # rows with batch -1: no segment
            a, b = max(s, c0), min(e, c1)
            if a < b:
                out["theta"][v][:, a - s:b - s] = onehot.T @ sG[:, a - c0:b - c0]
                out["logdelta"][v][:, a - s:b - s] = delta[:, a - s:b - s] * (onehot.T @ sQ[:, a - c0:b - c0])
    return out


@pytest.mark.parametrize("name,cols", [("mixed-257x161-k64", 4096), ("batch-unbatched-f32-k48-both", 64)])
def test_layer_scales_are_bitwise_what_they_were(name, cols):
    p = (DROPPED[name] if name in DROPPED else SHAPES[name])()
    a, b = layer_scales_before(p, cols), layer_scales(p, cols)
    assert a["loss"] == b["loss"]
    for k in ("mu", "logsigma", "g"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("theta", "logdelta"):
        assert len(a[k]) == len(b[k]) == len(p["batch_views"]) > 0
        for u, v in zip(a[k], b[k]):
            assert np.array_equal(u, v), k
