"""GPU: cusk_phen_rint against the rule restated in float64 (tests/test_prep_phen_rint_formats.py: rankdata, ndtri, mean and
population sd), and `prep-phen --rint` through the CLI.

rank2, n, the status and the NaN pattern are compared by equality.  The bound on `out` is max(ONE float32 ulp of the
reference, 8 n 2^-53).  The first term is the bound of tests/test_gpu_prep_phen.py: both sides round nearly the same
double (AS 241 and ndtri agree to about 1e-16 relative).  The second is n x unit round-off x a bound on |q| (|q| < 8 for
any n < 2^31): at the centre of an odd, tie-free trait q is exactly 0 and out = -m / s is the rounding residue of a sum that
is zero in exact arithmetic, and the two sides' residues differ.  Both are derived, not measured; the smallest gap between
adjacent scores, about 2.5 / n, is five orders above them at these sizes.  mean and sd are held to 8 n 2^-53 + 1e-14: the
same bound on a sum of n scores, plus sixteen-digit agreement of the two quantile functions on values below 8."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_prep_phen_rint_formats import OK, TOO_FEW, key_restated, rint_restated

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
POISON = -7.0
ARG = 2


@pytest.fixture(scope="module")
def eng():
    from cigwas_amd.skeleton import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tile():
    from cigwas_amd._lib import lib

    return int(lib().cusk_phen_rint_tile())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def trait_bytes(N, T):
    npad = T
    while npad < N:
        npad *= 2
    return 4 * (npad + N)


def run(eng, vals, select=None, offset=0.375, resident=None):
    """the call with a poisoned guard behind `out` and `rank2`; `resident`: the DeviceArray copy of vals to pass instead"""
    p, N = vals.shape
    out = np.full(p * N + GUARD, POISON, np.float32)
    rank2 = np.full(p * N + GUARD, 0xABCDABCD, np.uint32)
    got = eng.phen_rint(vals if resident is None else resident, N, p, select=select, offset=offset, out=out, stats={"rank2": rank2})
    assert np.all(out[p * N:] == POISON) and np.all(rank2[p * N:] == 0xABCDABCD)
    return got


def compare(got, ref, label):
    assert np.array_equal(got["status"], ref["status"]), (label, got["status"], ref["status"])
    assert np.array_equal(got["n"], ref["n"]), (label, got["n"], ref["n"])
    assert np.array_equal(got["rank2"].astype(np.int64), ref["rank2"]), label
    assert np.array_equal(np.isnan(got["out"]), np.isnan(ref["out"])) and np.array_equal(np.isinf(got["out"]), np.isinf(ref["out"])), label
    worst = 0.0
    for t in range(ref["out"].shape[0]):
        n = int(ref["n"][t])
        seen = np.isfinite(ref["out"][t])  # a trait that passes through may hold +-Inf
        if not seen.any():
            assert np.isnan(got["mean"][t]) and np.isnan(got["sd"][t])
            continue
        r = ref["out"][t, seen]
        bound = np.maximum(np.spacing(np.abs(r).astype(np.float32)).astype(np.float64), 8.0 * n * 2.0 ** -53)
        err = np.abs(got["out"][t, seen].astype(np.float64) - r)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (label, t, float((err / bound).max()))
        if np.isnan(ref["mean"][t]):  # passed through
            assert np.isnan(got["mean"][t]) and np.isnan(got["sd"][t])
            continue
        tol = 8.0 * n * 2.0 ** -53 + 1e-14
        assert abs(got["mean"][t] - ref["mean"][t]) <= tol and abs(got["sd"][t] - ref["sd"][t]) <= tol, (label, t)
    print(f"{label}: worst |out - float64| / bound = {worst:g}")


def properties(vals, got, label):
    """equal inputs give bitwise-equal outputs; the output is non-decreasing along the sorted input"""
    for t in range(vals.shape[0]):
        seen = ~np.isnan(got["out"][t])
        if not seen.any():
            continue
        k = key_restated(vals[t, seen])
        o = got["out"][t, seen]
        order = np.argsort(k, kind="stable")
        ks, os_ = k[order], o[order]
        same = np.diff(ks.astype(np.int64)) == 0
        assert np.all(_bits(os_)[1:][same] == _bits(os_)[:-1][same]), (label, t)
        assert np.all(np.diff(os_.astype(np.float64)) >= 0), (label, t)
        assert np.all(np.diff(os_.astype(np.float64))[~same] > 0), (label, t)  # distinct values keep distinct scores at these n


KINDS = ("continuous", "gaps30", "all_missing", "sorted", "reversed", "equal", "two_valued", "one_decimal", "signed_zeros",
         "denormals", "inf_missing", "lognormal")


def draw_kinds(N, seed):
    rng = np.random.default_rng(seed)
    V = np.empty((len(KINDS), N), np.float32)
    x = rng.standard_normal(N).astype(np.float32)
    V[0] = x
    V[1] = np.where(rng.random(N) < 0.3, np.nan, rng.standard_normal(N))
    V[2] = np.nan
    V[3] = np.sort(x)
    V[4] = np.sort(x)[::-1]
    V[5] = 4.25
    V[6] = rng.integers(0, 2, N) * 3.0 - 1.0
    V[7] = np.round(rng.standard_normal(N), 1)  # heavy ties, and both zeros: np.round gives -0.0
    V[8] = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], np.float32), N)
    V[9] = (rng.integers(-40, 41, N).astype(np.int64) * 1.401298464324817e-45).astype(np.float32)
    V[10] = rng.standard_normal(N)
    V[10, rng.random(N) < 0.2] = np.inf
    V[10, rng.random(N) < 0.2] = -np.inf
    V[11] = np.exp(2.0 * rng.standard_normal(N))
    return V


def sizes(T):
    return (1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 4 * T + 3)


@pytest.mark.parametrize("which", range(11))
def test_exact_ranks_values_and_properties_by_size(eng, tile, which):
    """every kind of input as one trait of one call, at the sizes around the tile: 2 T + 1 and 4 T + 3 need one and two merge
    stages across tiles"""
    from cigwas_amd.skeleton import DeviceArray

    N = sizes(tile)[which]
    V = draw_kinds(N, 100 + which)
    assert N < 1000 or np.any(np.signbit(V[7]) & (V[7] == 0))
    ref = rint_restated(V)
    got = run(eng, V)
    label = f"N={N}"
    compare(got, ref, label)
    properties(V, got, label)
    again = run(eng, V)
    assert np.array_equal(_bits(again["out"]), _bits(got["out"])) and np.array_equal(again["rank2"], got["rank2"])
    assert np.array_equal(again["mean"].view(np.uint64), got["mean"].view(np.uint64))
    assert np.array_equal(again["sd"].view(np.uint64), got["sd"].view(np.uint64))
    Vd = DeviceArray(V)
    try:
        res = run(eng, V, resident=Vd)
    finally:
        Vd.free()
    assert np.array_equal(_bits(res["out"]), _bits(got["out"])) and np.array_equal(res["rank2"], got["rank2"])
    # one trait alone gives the bytes it has among the others
    for t in (0, 7):
        one = run(eng, V[t:t + 1].copy())
        assert np.array_equal(_bits(one["out"][0]), _bits(got["out"][t])) and np.array_equal(one["rank2"][0], got["rank2"][t])


def test_many_traits_mixed_select_and_offsets(eng, tile):
    """p = 70, a different n per trait, every other third trait passed through; the three offsets"""
    N, p = tile + 1, 70
    rng = np.random.default_rng(7)
    V = rng.standard_normal((p, N)).astype(np.float32)
    V[::2] = np.round(V[::2], 2)
    for t in range(p):
        V[t, rng.random(N) < t / (p + 10.0)] = np.nan
    V[5, 100:] = np.nan
    V[6, 1:] = np.nan    # n = 1
    V[8, :] = -2.5       # constant
    V[9, 3] = np.inf     # passes through with its bits
    select = (np.arange(p) % 3 != 0).astype(np.uint8)
    select[6] = 1
    assert select[5] and select[8] and not select[9]
    ref = rint_restated(V, select)
    assert len(set(ref["n"])) > 60 and ref["status"][6] == TOO_FEW and ref["status"][8] == TOO_FEW and ref["n"][6] == 1
    got = run(eng, V, select=select)
    compare(got, ref, "p=70")
    properties(V[select.astype(bool)], {"out": got["out"][select.astype(bool)]}, "p=70")
    off = ~select.astype(bool)
    assert np.array_equal(_bits(got["out"][off]), _bits(V[off])) and not got["rank2"][off].any()
    assert np.all(got["status"][off] == OK) and np.all(np.isnan(got["mean"][off])) and np.all(np.isnan(got["sd"][off]))
    for t in (6, 8):
        assert np.all(np.isnan(got["out"][t])) and np.isnan(got["mean"][t]) and np.isnan(got["sd"][t])
    assert list(got["rank2"][8]) == [N + 1] * N
    for offset in (0.0, 0.375, 0.5):
        W = V[10:16]
        compare(run(eng, W, offset=offset), rint_restated(W, offset=offset), f"offset={offset}")
    # optional outputs may be absent
    from cigwas_amd._lib import lib

    out = np.full(6 * N + GUARD, POISON, np.float32)
    assert lib().cusk_phen_rint(eng.h, _ptr(np.ascontiguousarray(V[10:16])), N, 6, None, 0.375, _ptr(out), None, None, None, None, None) == 0
    assert np.array_equal(_bits(out[:6 * N].reshape(6, N)), _bits(run(eng, V[10:16])["out"])) and np.all(out[6 * N:] == POISON)


def test_groups_do_not_change_the_bytes(eng, tile):
    """engine option "phen_rint_bytes": p = 5 in groups of two gives the bytes of the single group"""
    rng = np.random.default_rng(11)
    try:
        for N in (65, 2 * tile + 1):
            V = np.round(rng.standard_normal((5, N)), 2).astype(np.float32)
            V[rng.random((5, N)) < 0.1] = np.nan
            select = np.array([1, 1, 0, 1, 1], np.uint8)
            eng.set_option("phen_rint_bytes", 1 << 30)
            whole, whole_sel = run(eng, V), run(eng, V, select=select)
            eng.set_option("phen_rint_bytes", 2 * trait_bytes(N, tile) + 8)
            for a, b in ((run(eng, V), whole), (run(eng, V, select=select), whole_sel)):
                assert np.array_equal(_bits(a["out"]), _bits(b["out"])) and np.array_equal(a["rank2"], b["rank2"])
                for key in ("mean", "sd"):
                    assert np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64))
                assert np.array_equal(a["n"], b["n"]) and np.array_equal(a["status"], b["status"])
            compare(whole, rint_restated(V), f"groups N={N}")
            # a single trait that does not fit is an argument error, and nothing is written
            eng.set_option("phen_rint_bytes", trait_bytes(N, tile) - 1)
            out = np.full(5 * N, POISON, np.float32)
            with pytest.raises(RuntimeError, match="phen_rint_bytes"):
                eng.phen_rint(V, N, 5, out=out)
            assert np.all(out == POISON)
        with pytest.raises(RuntimeError):
            eng.set_option("phen_rint_bytes", 0)
    finally:
        eng.set_option("phen_rint_bytes", 1 << 30)


def test_argument_errors_leave_the_outputs_alone(eng):
    from cigwas_amd._lib import lib

    L = lib()
    N, p = 50, 2
    V = np.random.default_rng(3).standard_normal((p, N)).astype(np.float32)
    out = np.full(p * N, POISON, np.float32)
    n = np.full(p, -5, np.int32)
    rank2 = np.full(p * N, 77, np.uint32)
    for args in ((None, N, p, None, 0.375, _ptr(out)), (_ptr(V), N, p, None, 0.375, None), (_ptr(V), 0, p, None, 0.375, _ptr(out)),
                 (_ptr(V), N, 0, None, 0.375, _ptr(out)), (_ptr(V), 1 << 31, p, None, 0.375, _ptr(out)),
                 (_ptr(V), N, p, None, -0.001, _ptr(out)), (_ptr(V), N, p, None, 0.5000001, _ptr(out)),
                 (_ptr(V), N, p, None, float("nan"), _ptr(out))):
        assert L.cusk_phen_rint(eng.h, *args, _ptr(n), None, None, None, _ptr(rank2)) == ARG, args
        assert L.cusk_last_error(eng.h).decode().startswith("cusk_phen_rint")
    assert L.cusk_phen_rint(None, _ptr(V), N, p, None, 0.375, _ptr(out), _ptr(n), None, None, None, _ptr(rank2)) == ARG
    assert np.all(out == POISON) and np.all(n == -5) and np.all(rank2 == 77)
    compare(run(eng, V), rint_restated(V), "after the errors")


# ---- through the command line ---------------------------------------------------------------------------------------

def _cli(*argv):
    return subprocess.run([sys.executable, "-c", "import sys, cigwas_amd.cli as c; c.main(sys.argv[1:])", *argv], cwd=ROOT,
                          capture_output=True, text=True)


def _skew(x):
    x = x.astype(np.float64)
    d = x - x.mean()
    return float((d ** 3).mean() / (d ** 2).mean() ** 1.5)


def test_cli_prep_phen_rint(eng, tmp_path):
    import cigwas_amd as cg

    N = 300
    rng = np.random.default_rng(21)
    age = rng.uniform(40, 70, N)
    bio = np.exp(0.03 * (age - 55) + 0.9 * rng.standard_normal(N))  # log-normal around a covariate effect
    grade = np.digitize(rng.standard_normal(N), [-0.4, 0.8]).astype(np.float64)
    Y = np.vstack([bio, grade]).astype(np.float32)
    Y[0, rng.random(N) < 0.05] = np.nan
    X = age[None, :].astype(np.float32)
    names, absent = ["bio", "grade"], 17
    stem = str(tmp_path / "set")
    with open(stem + ".fam", "w") as f:
        f.writelines(f"f{i} i{i} 0 0 {1 + i % 2} -9\n" for i in range(N))
    table, covar = str(tmp_path / "traits.tsv"), str(tmp_path / "covar.tsv")
    for path, cols, M, skip in ((table, names, Y, absent), (covar, ["age"], X, -1)):
        with open(path, "w") as f:
            f.write("IID\tFID\t" + "\t".join(cols) + "\n")
            for i in rng.permutation(N):
                if i != skip:
                    f.write(f"i{i}\tf{i}\t" + "\t".join("NA" if np.isnan(v) else repr(float(v)) for v in M[:, i]) + "\n")
    Ya = Y.copy()
    Ya[:, absent] = np.nan
    adjust, select = np.array([1, 0], np.uint8), np.array([1, 0], np.uint8)
    step1 = eng.phen_adjust(Ya, X, N, 2, 1, adjust=adjust)
    step2 = eng.phen_rint(step1["out"], N, 2, select=select, ranks=True)
    assert np.all(step1["status"] == OK) and np.all(step2["status"] == OK)

    out_rint, out_plain, out_half = str(tmp_path / "rint.phen"), str(tmp_path / "plain.phen"), str(tmp_path / "half.phen")
    for path, flags in ((out_rint, ["--rint"]), (out_plain, []), (out_half, ["--rint", "--rint-offset", "0.5"])):
        r = _cli("prep-phen", stem, table, path, "--covar", covar, "--ordinal", "grade", *flags)
        assert r.returncode == 0, r.stdout + r.stderr
    _n, d_rint, info = cg.phen_table_load(out_rint, stem + ".fam")
    _n, d_plain, _i = cg.phen_table_load(out_plain, stem + ".fam")
    _n, d_half, _i = cg.phen_table_load(out_half, stem + ".fam")
    assert _n == names and info == {"matched": N, "dropped": 0, "in_order": True}
    same = lambda a, b: bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))  # noqa: E731
    assert same(d_rint, step2["out"])
    assert same(d_half, eng.phen_rint(step1["out"], N, 2, select=select, offset=0.5)["out"]) and not same(d_half[0], d_rint[0])
    assert same(d_rint[1], d_plain[1]) and same(d_plain, step1["out"])
    compare(step2, rint_restated(step1["out"], select), "cli")
    # without the flag: byte for byte the file of the phen_adjust route
    route = str(tmp_path / "route.phen")
    cg.phen_write(route, stem + ".fam", names, step1["out"])
    assert open(out_plain, "rb").read() == open(route, "rb").read()
    for path in (out_rint, out_plain, out_half):
        r = _cli("check-phen", stem, path)
        assert r.returncode == 0, r.stdout + r.stderr
    rep = [ln.split("\t") for ln in open(out_rint + ".prep.tsv").read().splitlines()]
    assert rep[0] == ["trait", "mode", "n", "mean", "sd", "r2", "rint_mean", "rint_sd"]
    assert [x[1] for x in rep[1:]] == ["adjusted+rint", "standardised"] and rep[2][6:] == ["NA", "NA"]
    assert abs(float(rep[1][6]) - step2["mean"][0]) <= 1e-8 and abs(float(rep[1][7]) - step2["sd"][0]) <= 1e-8 * step2["sd"][0]
    rep = [ln.split("\t") for ln in open(out_plain + ".prep.tsv").read().splitlines()]
    assert rep[0] == ["trait", "mode", "n", "mean", "sd", "r2"] and [x[1] for x in rep[1:]] == ["adjusted", "standardised"]
    # without covariates the mode is "rint"
    out_nc = str(tmp_path / "nc.phen")
    r = _cli("prep-phen", stem, table, out_nc, "--rint")
    assert r.returncode == 0, r.stdout + r.stderr
    assert [ln.split("\t")[1] for ln in open(out_nc + ".prep.tsv").read().splitlines()[1:]] == ["rint", "rint"]
    # the transform removes the skew the residual keeps (a comparison of the two, not a threshold)
    seen = ~np.isnan(d_plain[0])
    s_plain, s_rint = _skew(d_plain[0, seen]), _skew(d_rint[0, seen])
    print(f"skewness of bio: residual {s_plain:.4f}, transformed {s_rint:.4f}")
    assert abs(s_rint) < abs(s_plain)
    # argument errors before the device is asked for; a trait that cannot be ranked is named and nothing is written
    assert _cli("prep-phen", stem, table, str(tmp_path / "x.phen"), "--rint-offset", "0.3").returncode != 0
    assert _cli("prep-phen", stem, table, str(tmp_path / "x.phen"), "--rint", "--rint-offset", "0.6").returncode != 0
    assert not os.path.exists(str(tmp_path / "x.phen"))
