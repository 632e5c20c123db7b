"""`prep-phen` / `check-phen` without a GPU: the symbols and their signatures, the argv of the native commands and the
argument errors, the table reader, the alignment to a .fam and the .phen writer through the host-only ABI, and the rule of
cusk_phen_adjust (include/cusk_hip.h) restated in numpy float64 (`adjust_restated`, which tests/test_gpu_prep_phen.py
imports as its reference) with the properties a least-squares residual must have.

The golden small.phen and with_nan.phen have no FID / IID header (the reference's loader skips whatever the first line is),
so the reader must refuse them as they are; their values are checked under a proper header, against the loader's semantics
((float)atof per token, NA -> NaN, rows as they come)."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = os.path.join(ROOT, "tests", "golden", "files")
MAX_COVAR, CHUNK, PIVOT_MIN = 63, 4096, 1e-8
OK, SINGULAR, TOO_FEW = 0, 1, 2


# ---- the rule, restated ---------------------------------------------------------------------------------------------

def unit_pivots(G):
    """pivots of the Cholesky factorisation of D^-1/2 G D^-1/2 (unit diagonal): 1 - R^2 of column j on the earlier ones;
    None where the diagonal of G is not positive.  Stops at the first pivot below PIVOT_MIN."""
    d = np.diag(G).copy()
    if not np.all(d > 0):
        return None
    S = G / np.sqrt(np.outer(d, d))
    np.fill_diagonal(S, 1.0)
    k = len(d)
    piv = np.zeros(k)
    for j in range(k):
        piv[j] = S[j, j]
        if not piv[j] >= PIVOT_MIN:
            return piv[:j + 1]
        S[j:, j] /= np.sqrt(piv[j])
        S[j, j] = np.sqrt(piv[j])
        for m in range(j + 1, k):
            S[m:, m] -= S[m:, j] * S[m, j]
    return piv


def adjust_restated(Y, X=None, adjust=None):
    """cusk_phen_adjust in numpy float64: dict(out float32 p x N, n, mean, sd, beta p x (c + 1) raw units, r2, status, cond
    -- the condition number of the scaled design per adjusted trait).  The fit is np.linalg.lstsq on the RAW covariates with
    an intercept; the status is the rule's (pivots of the unit-diagonal Gram of the scaled design)."""
    Y = np.asarray(Y, np.float32).astype(np.float64)
    p, N = Y.shape
    X = np.zeros((0, N)) if X is None else np.asarray(X, np.float32).astype(np.float64).reshape(-1, N)
    c = X.shape[0]
    adjust = np.ones(p, bool) if adjust is None else np.asarray(adjust).astype(bool)
    A = np.all(np.isfinite(X), axis=0) if c else np.ones(N, bool)
    if c:
        mu = X[:, A].mean(axis=1) if A.any() else np.full(c, np.nan)
        sigma = np.sqrt(((X[:, A] - mu[:, None]) ** 2).mean(axis=1)) if A.any() else np.full(c, np.nan)
        for j in range(c):
            if not sigma[j] > 0:
                raise ValueError(f"covariate {j} is constant")
    res = {"out": np.full((p, N), np.nan, np.float32), "n": np.zeros(p, np.int32), "mean": np.full(p, np.nan), "sd": np.full(p, np.nan),
           "beta": np.full((p, c + 1), np.nan), "r2": np.full(p, np.nan), "status": np.zeros(p, np.int32), "cond": np.full(p, np.nan)}
    for t in range(p):
        adj = bool(c and adjust[t])
        U = np.isfinite(Y[t]) & (A if adj else True)
        n = int(U.sum())
        res["n"][t] = n
        y = Y[t, U]
        e, status = y, OK
        if adj:
            if n < c + 2:
                status = TOO_FEW
            else:
                Zs = np.vstack([np.ones(n), (X[:, U] - mu[:, None]) / sigma[:, None]]).T
                piv = unit_pivots(Zs.T @ Zs)
                if piv is None or not np.all(piv >= PIVOT_MIN):
                    status = SINGULAR
                else:
                    res["cond"][t] = np.linalg.cond(Zs)
                    Z = np.vstack([np.ones(n), X[:, U]]).T
                    beta = np.linalg.lstsq(Z, y, rcond=None)[0]
                    e = y - Z @ beta
        elif n < 2:
            status = TOO_FEW
        if status == OK:
            m = e.sum() / n
            s = np.sqrt(((e - m) ** 2).sum() / n)
            if not s > 0:
                status = TOO_FEW
        res["status"][t] = status
        if status != OK:
            continue
        res["mean"][t], res["sd"][t] = m, s
        res["out"][t, U] = ((e - m) / s).astype(np.float32)
        if adj:
            res["beta"][t] = beta
            res["r2"][t] = 1.0 - (e ** 2).sum() / ((y - y.mean()) ** 2).sum()
    return res


def premise_holds(ref, c):
    """the bound of the GPU comparison rests on kappa(scaled design)^2 * c * n * 2^-53 < 2^-26"""
    k = ref["cond"][np.isfinite(ref["cond"])]
    n = ref["n"][np.isfinite(ref["cond"])]
    return bool(np.all(k ** 2 * max(c, 1) * n * 2.0 ** -53 < 2.0 ** -26))


def draw(N, p, c, seed, gaps=None, age=False):
    """traits that depend on the covariates, float32.  gaps: None, "random" (30 % per trait), "first_chunk" (trait 0 only on
    the first CHUNK individuals), "covar" (covariate 0 missing for 10 %), "all_nan" (the last trait has no value)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((c, N))
    if age and c >= 2:
        X[0] = rng.uniform(40, 70, N)
        X[1] = X[0] ** 2
    X = X.astype(np.float32)
    w = rng.standard_normal((p, c)) / max(1.0, np.sqrt(c))
    Xs = (X - X.mean(axis=1, keepdims=True)) / np.where(X.std(axis=1, keepdims=True) > 0, X.std(axis=1, keepdims=True), 1.0) if c else X
    Y = (w @ Xs + rng.standard_normal((p, N)) * 0.7 + rng.uniform(-3, 3, (p, 1))).astype(np.float32)
    if gaps == "random":
        Y[rng.random((p, N)) < 0.3] = np.nan
    elif gaps == "first_chunk":
        Y[0, CHUNK:] = np.nan
    elif gaps == "covar" and c:
        X[0, rng.random(N) < 0.1] = np.nan
    elif gaps == "all_nan":
        Y[-1] = np.nan
    return Y, X


# ---- symbols and command lines --------------------------------------------------------------------------------------

NEW_SYMBOLS = ("cusk_phen_adjust", "cusk_phen_moments", "cusk_phen_timing", "cusk_phen_table_load", "cusk_phen_table_rows",
               "cusk_phen_table_cols", "cusk_phen_table_name", "cusk_phen_table_data", "cusk_phen_table_matched",
               "cusk_phen_table_dropped", "cusk_phen_table_in_order", "cusk_phen_table_free", "cusk_phen_write")


def test_symbols_exist_with_the_headers_signatures():
    from cigwas_amd._lib import SYMBOLS, lib

    header = open(os.path.join(ROOT, "include", "cusk_hip.h")).read()
    L = lib()
    for name in NEW_SYMBOLS:
        assert name in SYMBOLS and hasattr(L, name), name
        decl = re.search(r"\b" + name + r"\(([^;]*?)\);", header, re.S)
        assert decl, name
        args = [a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(SYMBOLS[name][1]) == len(args), (name, args)
    assert re.search(r"#define CUSK_PHEN_MAX_COVAR 63\b", header) and re.search(r"#define CUSK_PHEN_CHUNK %d\b" % CHUNK, header)
    assert "POPULATION" in header and "CUSK_PHEN_PIVOT_MIN 1e-8" in header
    # the three entry points that need no device answer argument errors without one
    assert L.cusk_phen_adjust(None, None, None, 0, 0, 0, None, None, None, None, None, None, None, None) == 2
    assert L.cusk_phen_moments(None, None, 0, 0, None, None, None) == 2


def _args(**kw):
    base = dict(bfiles="set", table="t.tsv", out="o.phen", covar=None, ordinal=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_argv_and_argument_errors(tmp_path):
    from cigwas_amd import cli

    assert cli.prep_phen_argv(_args()) == [cli.MPS_PATH, "prep-phen", "set", "t.tsv", "o.phen", "NULL"]
    assert cli.prep_phen_argv(_args(covar="c.tsv")) == [cli.MPS_PATH, "prep-phen", "set", "t.tsv", "o.phen", "c.tsv"]
    assert cli.check_phen_argv(argparse.Namespace(bfiles="set", phen="x.phen")) == [cli.MPS_PATH, "check-phen", "set", "x.phen"]
    table = tmp_path / "t.tsv"
    table.write_text("IID FID a b cc\n1 1 0.5 1 0\n2 2 0.25 0 1\n3 3 NA 1 2\n")
    argv = cli.prep_phen_argv(_args(table=str(table), ordinal="cc,2"))
    assert argv[-1] == "ordinal=3,2"
    # through the parser
    a = cli.build_parser().parse_args(["prep-phen", "set", str(table), "o.phen", "--covar", "c.tsv", "--ordinal", "b"])
    assert a.func is cli.prep_phen and cli.prep_phen_argv(a)[5:] == ["c.tsv", "ordinal=2"]
    a = cli.build_parser().parse_args(["check-phen", "set", "x.phen"])
    assert a.func is cli.check_phen
    for bad in (_args(out="t.tsv"), _args(covar="c.tsv", out="c.tsv"), _args(out="set.fam"),
                _args(table=str(table), ordinal="nope"), _args(table=str(table), ordinal="4"), _args(table=str(table), ordinal="b,b")):
        with pytest.raises(SystemExit) as ex:
            cli.prep_phen_argv(bad)
        assert ex.value.code not in (0, None)
    link = tmp_path / "link.tsv"
    os.symlink(table, link)
    with pytest.raises(SystemExit):
        cli.prep_phen_argv(_args(table=str(table), out=str(link)))  # another spelling of TABLE
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["prep-phen", "set"])


# ---- reader, aligner, writer ----------------------------------------------------------------------------------------

def fam_ids(path):
    return [ln.split()[:2] for ln in open(path) if ln.split()]


def write_table(path, ids, names, values, header=("FID", "IID"), eol="\n"):
    """values: rows x cols of strings or floats"""
    with open(path, "w", newline="") as f:
        f.write("\t".join(list(header) + list(names)) + eol)
        for (fid, iid), row in zip(ids, values):
            first = (fid, iid) if header[0] == "FID" else (iid, fid)
            f.write("\t".join(list(first) + [v if isinstance(v, str) else repr(float(v)) for v in row]) + eol)


def test_golden_files_values_under_a_header_and_refusal_without(tmp_path, oracle):
    from cigwas_amd import phen_table_load

    for name in ("small.phen", "with_nan.phen"):
        with pytest.raises(ValueError, match="line 1"):
            phen_table_load(os.path.join(FILES, name))
    # with_nan.phen: its rows under a header; nan and NA both read as missing
    lines = open(os.path.join(FILES, "with_nan.phen")).read().splitlines()
    width = len(lines[1].split()) - 2
    path = tmp_path / "with_nan.tsv"
    path.write_text("\n".join(["FID IID " + " ".join(f"t{j}" for j in range(width))] + lines[1:]) + "\n")
    n, p, want = oracle.load_phen(os.path.join(FILES, "with_nan.phen"))
    names, data, info = phen_table_load(str(path))
    assert (len(names), data.shape) == (p, (p, n)) and info["matched"] == n
    assert np.array_equal(data.view(np.uint32) & 0x7FFFFFFF == 0x7FC00000, np.isnan(want.reshape(p, n)))
    assert np.array_equal(data, want.reshape(p, n), equal_nan=True) and np.isnan(want).any()
    # small.phen: one value per line of small.fam; as a trait column of a table it aligns to the .fam one to one
    fam = os.path.join(FILES, "small.fam")
    ids = fam_ids(fam)
    tokens = open(os.path.join(FILES, "small.phen")).read().split()
    assert len(tokens) == len(ids)
    write_table(tmp_path / "small.tsv", ids, ["y"], [[t] for t in tokens])
    names, data, info = phen_table_load(str(tmp_path / "small.tsv"), fam)
    assert names == ["y"] and info == {"matched": len(ids), "dropped": 0, "in_order": True}
    assert np.array_equal(data[0], np.array([np.float32(float(t)) for t in tokens]))


def test_alignment_shuffled_missing_extra_header_forms_and_errors(tmp_path):
    from cigwas_amd import phen_table_load

    fam = os.path.join(FILES, "small.fam")
    ids = fam_ids(fam)
    N = len(ids)
    rng = np.random.default_rng(5)
    vals = rng.standard_normal((N, 3)).astype(np.float32)
    vals[2, 1] = np.nan
    rows = [[("NA" if np.isnan(v) else repr(float(v))) for v in r] for r in vals]
    names = ["a", "b", "c"]
    want = vals.T
    perm = rng.permutation(N)
    for label, header, eol in (("plain", ("FID", "IID"), "\n"), ("swapped", ("IID", "FID"), "\n"), ("eid", ("FID", "EID"), "\n"),
                               ("crlf", ("EID", "FID"), "\r\n")):
        path = str(tmp_path / f"{label}.tsv")
        fake = [(f"fam{i}", iid) for i, (_f, iid) in enumerate(ids)]  # the FID column is not what rows are matched by
        write_table(path, [fake[i] for i in perm], names, [rows[i] for i in perm], header=header, eol=eol)
        got_names, data, info = phen_table_load(path, fam)
        assert got_names == names and np.array_equal(data, want, equal_nan=True), label
        assert info == {"matched": N, "dropped": 0, "in_order": False}
        _names, as_is, info2 = phen_table_load(path)
        assert np.array_equal(as_is, want[:, perm], equal_nan=True) and info2["matched"] == N
    # two individuals missing, two extra
    keep = [i for i in range(N) if i not in (1, 6)]
    extra = [("x", "extra1"), ("x", "extra2")]
    write_table(tmp_path / "gaps.tsv", [ids[i] for i in keep] + extra, names, [rows[i] for i in keep] + [["1", "2", "3"]] * 2)
    _n, data, info = phen_table_load(str(tmp_path / "gaps.tsv"), fam)
    assert info == {"matched": N - 2, "dropped": 2, "in_order": False}
    assert np.all(np.isnan(data[:, [1, 6]])) and np.array_equal(data[:, keep], want[:, keep], equal_nan=True)
    # header only: a table without rows, everybody NA
    (tmp_path / "head.tsv").write_text("FID IID a b\n")
    got_names, data, info = phen_table_load(str(tmp_path / "head.tsv"), fam)
    assert got_names == ["a", "b"] and data.shape == (2, N) and np.all(np.isnan(data)) and info["matched"] == 0
    # errors: each names its line
    cases = {"dup": ("FID IID a\n1 7 0.5\n2 8 1\n3 7 2\n", "line 4.*duplicate IID 7"),
             "token": ("FID IID a b\n1 7 0.5 1\n2 8 1 1.5x\n", "line 3, column 4 \\(b\\).*1.5x"),
             "ragged": ("FID IID a b\n1 7 0.5 1\n2 8 1\n", "line 3.*3 columns"),
             "noids": ("id a b\n1 2 3\n", "line 1"), "empty": ("", "empty")}
    for label, (text, pattern) in cases.items():
        (tmp_path / f"{label}.tsv").write_text(text)
        with pytest.raises(ValueError, match=pattern):
            phen_table_load(str(tmp_path / f"{label}.tsv"), fam)
    with pytest.raises(ValueError):
        phen_table_load(str(tmp_path / "absent.tsv"))
    # a line of 10^5 characters
    wide = [f"v{j}" for j in range(20000)]
    (tmp_path / "wide.tsv").write_text("FID IID " + " ".join(wide) + "\n" + ids[0][0] + " " + ids[0][1] + " " + " ".join(["0.25"] * 20000) + "\n")
    got_names, data, info = phen_table_load(str(tmp_path / "wide.tsv"), fam)
    assert len(got_names) == 20000 and np.all(data[:, 0] == 0.25) and np.all(np.isnan(data[:, 1:]))


def test_writer_round_trips_float32_bit_for_bit(tmp_path, oracle):
    from cigwas_amd import phen_table_load, phen_write

    rng = np.random.default_rng(11)
    N, p = 2500, 4
    bits = rng.integers(0, 2 ** 32, N * p, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32).copy()
    v[~np.isfinite(v)] = np.nan  # Inf and NaN payloads are NA in a .phen
    v[:6] = [np.float32(1e-45), -np.float32(1e-45), np.float32(1.17549421e-38), np.finfo(np.float32).max, -np.finfo(np.float32).max, 0.0]
    v[6] = np.nan
    assert (np.abs(v[np.isfinite(v)]) < np.finfo(np.float32).tiny).sum() > 10  # denormals are in
    data = v.reshape(p, N)
    fam = tmp_path / "x.fam"
    fam.write_text("".join(f"f{i}\ti{i} 0 0 1 -9\n" for i in range(N)))
    out = tmp_path / "x.phen"
    phen_write(str(out), str(fam), ["a", "b", "c", "d"], data)
    text = open(out).read().splitlines()
    assert text[0] == "FID\tIID\ta\tb\tc\td" and len(text) == N + 1 and text[1].split("\t")[:2] == ["f0", "i0"]
    assert "NA" in text[7].split("\t") or "NA" in open(out).read()
    n2, p2, got = oracle.load_phen(str(out))  # the reference loader's semantics: NA -> NaN, (float)atof
    assert (n2, p2) == (N, p)
    same = got.reshape(p, N).view(np.uint32) == data.view(np.uint32)
    assert np.all(same | (np.isnan(got.reshape(p, N)) & np.isnan(data)))
    names, back, info = phen_table_load(str(out), str(fam))
    assert names == ["a", "b", "c", "d"] and info["in_order"]
    assert np.all((back.view(np.uint32) == data.view(np.uint32)) | (np.isnan(back) & np.isnan(data)))
    with pytest.raises(RuntimeError):
        phen_write(str(fam), str(fam), ["a", "b", "c", "d"], data)  # would overwrite the .fam
    with pytest.raises(RuntimeError):
        phen_write(str(out), str(fam), ["a"], data[:1, :10])  # not one row per individual
    with pytest.raises(RuntimeError):
        phen_write(str(tmp_path / "no_such_dir" / "x.phen"), str(fam), ["a", "b", "c", "d"], data)


# ---- the restated rule has the properties of the thing it restates ---------------------------------------------------

def test_restated_rule_properties():
    Y, X = draw(700, 3, 4, 1, gaps="random")
    X[2, ::17] = np.nan
    X[1] = np.round(4 * X[1])  # small integers: 8 x - 3 below is exact in float32
    # c = 0 is plain standardisation
    r0 = adjust_restated(Y)
    for t in range(3):
        U = np.isfinite(Y[t])
        y = Y[t, U].astype(np.float64)
        assert np.array_equal(r0["out"][t, U], ((y - y.mean()) / y.std()).astype(np.float32)) and np.all(np.isnan(r0["out"][t, ~U]))
    assert np.all(r0["status"] == OK) and np.all(np.isnan(r0["r2"]))
    # adjust flag off: the same values as without covariates
    r_off = adjust_restated(Y, X, adjust=[0, 0, 0])
    assert np.array_equal(r_off["out"], r0["out"], equal_nan=True)
    # residuals: orthogonal to the constant and to every covariate on U_t, mean 0, population sd 1
    r = adjust_restated(Y, X)
    assert np.all(r["status"] == OK) and premise_holds(r, 4)
    A = np.all(np.isfinite(X), axis=0)
    for t in range(3):
        U = A & np.isfinite(Y[t])
        assert r["n"][t] == U.sum() and np.all(np.isnan(r["out"][t, ~U]))
        e = r["out"][t, U].astype(np.float64)
        assert abs(e.mean()) < 1e-6 and abs(e.std() - 1) < 1e-6
        for j in range(4):
            x = X[j, U].astype(np.float64)
            assert abs(np.dot(e, x - x.mean())) / (len(e) * x.std()) < 1e-6
        assert 0 < r["r2"][t] < 1
    # an affine change of a covariate changes nothing but its coefficient
    X2 = X.astype(np.float64)
    X2[1] = 8.0 * X2[1] - 3.0
    r2 = adjust_restated(Y, X2.astype(np.float32))
    ulp = np.spacing(np.abs(r["out"]))
    assert np.all((np.abs(r2["out"] - r["out"]) <= ulp) | np.isnan(r["out"]))
    assert np.allclose(r2["beta"][:, 2] * 8.0, r["beta"][:, 2], rtol=1e-6)
    # status 1: a duplicated covariate; a covariate constant on one trait's individuals only
    dup = np.vstack([X[:2], X[:1]])
    assert np.all(adjust_restated(Y, dup)["status"] == SINGULAR)
    Xc = X[:2].copy()
    Yc = Y.copy()
    Xc[0, :300] = 2.0
    Yc[1, 300:] = np.nan  # trait 1 lives where covariate 0 does not vary
    rc = adjust_restated(Yc, Xc)
    assert list(rc["status"]) == [OK, SINGULAR, OK] and np.all(np.isnan(rc["out"][1]))
    # status 2: n_t = c + 1; and a trait without values
    Yf = Y.copy()
    full = np.flatnonzero(np.all(np.isfinite(X), axis=0) & np.isfinite(Y[0]))
    Yf[0] = np.nan
    Yf[0, full[:5]] = Y[0, full[:5]]
    Yf[2] = np.nan
    rf = adjust_restated(Yf, X)
    assert list(rf["status"]) == [TOO_FEW, OK, TOO_FEW] and list(rf["n"][[0, 2]]) == [5, 0]
    Yf[0, full[5]] = Y[0, full[5]]
    assert adjust_restated(Yf, X)["status"][0] == OK  # c + 2 individuals are enough
    with pytest.raises(ValueError, match="covariate 1"):
        adjust_restated(Y, np.vstack([X[:1], np.full((1, 700), 3.0, np.float32)]))
