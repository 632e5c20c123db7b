#!/usr/bin/env python3
"""Golden vectors for `iv-candidates` / `check-ivs`: seeded merged skeletons and what the REFERENCE ITSELF makes of them.

Run in the build container only: imports /root/reference/cusk_postprocessing/check_mr_assumptions.py (never copied,
never shipped), calls its `get_iv_candidates` and `check_ivs` on files written here and records DATA only:

  iv_check_kat.json      per case: seed, shape, N, both alphas, margin, d and the row counts (small, readable)
  iv_check_<case>.npz    per case: the candidate rows and the rows of every stored flag combination (`candidates`,
                         `rows_<combination>`; sorted: exposure, outcome, IV); the three input files' text as bytes
                         (`input_mdim`, `input_sam`, `input_scm`) for the small cases, for the large ones the dense
                         `adj` / `corr` the files were written from (mmwrite of these arrays reproduces the files;
                         checked here by reading them back); and every distinct test the reference performed -- x, y,
                         the conditioning set (an index into a list of sets, -1 = empty), which alpha, z_ref and the
                         threshold -- heard while the reference's check_ivs ran its own, untouched `_indep`: a wrapper
                         notes each call's arguments, pass-through wrappers around `_fisher_z` and `_alpha_thr` keep
                         the values they returned

margin = min |z_ref - thr| over all tests of the case, d = max |z_ref - z_schur| with z_schur the package's float64
numpy Schur form (cigwas_amd.ivcheck.host_z).  The seed of a case is advanced until
  * every stored flag combination is non-trivial (cases with p >= 3): some rows kept, some candidates rejected,
  * both verdicts occur among the marginal and among the conditional tests,
  * margin >= 1000 d,
so no test has to leave an item out.  A seed is first screened with the package's host form (fast) and then confirmed by
the reference; the assertions are on the reference's results.

Usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_iv_check_golden.py [/root/reference]
"""
import json
import os
import sys
import tempfile

import numpy as np
import scipy.sparse as sp
from scipy.io import mmread, mmwrite

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from cusk_postprocessing import check_mr_assumptions as ref  # noqa: E402

from cigwas_amd import ivcheck  # noqa: E402
from cigwas_amd.synth import merged_skeleton  # noqa: E402  (the same generator the tests use)

ALL_FLAGS = [(False, False), (True, False), (False, True), (True, True)]  # (relaxed_local_faithfulness, check_reverse_causality)
CASES = [
    # name, first seed, traits, markers, N, noise, accept_alpha, reject_alpha, flag combinations, inputs as text
    ("p2", 101, 2, 12, 10000, 0.002, 1e-2, 5e-2, ALL_FLAGS, True),
    ("p6", 201, 6, 40, 20000, 0.002, 1e-4, 1e-3, ALL_FLAGS, True),
    ("p14", 301, 14, 300, 50000, 0.002, 1e-4, 1e-3, ALL_FLAGS, True),
    ("p40", 401, 40, 200, 100000, 0.002, 1e-4, 1e-3, ALL_FLAGS, False),
    ("p66", 501, 66, 40, 100000, 0.001, 1e-4, 1e-3, ALL_FLAGS, False),
    ("p128", 601, 128, 40, 200000, 0.001, 1e-4, 1e-3, [(False, False), (True, False)], False)  # no reverse pass: its 1-trait
    # sets are covered by the other cases and would be most of this file,
]
ONLY = os.environ.get("IV_GOLDEN_ONLY")  # comma-separated case names: regenerate these, keep the others


def text(path):
    with open(path) as f:
        return f.read()


def sort_rows(df):
    if len(df) == 0:
        return []
    return sorted((int(e), int(o), int(v)) for e, o, v in zip(df["Exposure"], df["Outcome"], df["IV"]))


class Recorder:
    """Listens to the reference's own `_indep`: notes the arguments of a call, lets the untouched function run, and picks
    up the z and the threshold it computed from pass-through wrappers around `_fisher_z` and `_alpha_thr`.  A call with
    arguments seen before is answered with the verdict the reference gave the first time (its check_ivs repeats the same
    test for every exposure)."""

    def __init__(self):
        self.tests, self.seen = {}, {}
        self.orig = (ref._indep, ref._fisher_z, ref._alpha_thr)

    def __enter__(self):
        indep, fisher_z, alpha_thr = self.orig

        def fisher_z_heard(*a, **k):
            self.seen["z"] = fisher_z(*a, **k)
            return self.seen["z"]

        def alpha_thr_heard(*a, **k):
            self.seen["thr"] = alpha_thr(*a, **k)
            return self.seen["thr"]

        def indep_heard(x_ix, y_ix, s_ixs, corr, sample_size, alpha):
            key = (int(x_ix), int(y_ix), tuple(int(s) for s in s_ixs), float(alpha))
            if key not in self.tests:
                self.seen.clear()
                verdict = bool(indep(x_ix, y_ix, s_ixs, corr, sample_size, alpha))
                zr, thr = float(self.seen["z"]), float(self.seen["thr"])
                assert verdict == (zr < thr)
                self.tests[key] = (zr, thr)
            zr, thr = self.tests[key]
            return zr < thr

        ref._indep, ref._fisher_z, ref._alpha_thr = indep_heard, fisher_z_heard, alpha_thr_heard
        return self

    def __exit__(self, *exc):
        ref._indep, ref._fisher_z, ref._alpha_thr = self.orig


def screen(stem, N, a_acc, a_rej, flags, ncand, p):
    """the package's host form: cheap look at whether this seed can satisfy the non-triviality conditions"""
    for relaxed, rev in flags:
        rows = ivcheck.check_ivs(stem, N, a_acc, a_rej, relaxed_local_faithfulness=relaxed, check_reverse_causality=rev)
        if p >= 3 and not (0 < len(rows) < ncand):
            return False
    return True


def run_case(name, seed, p, m, N, noise, a_acc, a_rej, flags, as_text):
    adj, corr, ixs, _ = merged_skeleton(seed, p, m, noise=noise)
    n = p + m
    with tempfile.TemporaryDirectory() as d:
        stem = os.path.join(d, "all_merged")
        mmwrite(stem + "_sam.mtx", sp.coo_matrix(adj.astype(np.int32)))
        mmwrite(stem + "_scm.mtx", sp.coo_matrix(corr))
        with open(stem + ".mdim", "w") as f:
            f.write(f"{n}\t{p}\t3\n")
        back = mmread(stem + "_scm.mtx").toarray()
        np.fill_diagonal(back, 1.0)
        assert np.array_equal(back, corr), "the matrix-market text does not reproduce the correlations"
        cand = sort_rows(ref.get_iv_candidates(stem))
        if not screen(stem, N, a_acc, a_rej, flags, len(cand), p):
            return None
        with Recorder() as rec:
            rows = {}
            for relaxed, rev in flags:
                rows[f"relaxed={int(relaxed)},reverse={int(rev)}"] = sort_rows(
                    ref.check_ivs(stem, N, a_acc, a_rej, relaxed_local_faithfulness=relaxed, check_reverse_causality=rev))
        inputs = {"mdim": text(stem + ".mdim"), "sam": text(stem + "_sam.mtx"), "scm": text(stem + "_scm.mtx")} if as_text else None
    # the distinct tests as arrays
    set_ids, set_lists = {}, []
    tx, ty, ts, ta, tz, tt = [], [], [], [], [], []
    for (x, y, S, alpha), (zr, thr) in rec.tests.items():
        sid = -1
        if S:
            if S not in set_ids:
                set_ids[S] = len(set_lists)
                set_lists.append(S)
            sid = set_ids[S]
        tx.append(x), ty.append(y), ts.append(sid), tz.append(zr), tt.append(thr)
        ta.append(0 if alpha == a_acc else 1)
    tx, ty, ts, ta = (np.array(a, np.int32) for a in (tx, ty, ts, ta))
    tz, tt = np.array(tz), np.array(tt)
    set_off = np.zeros(len(set_lists) + 1, np.int32)
    set_off[1:] = np.cumsum([len(s) for s in set_lists])
    sets = np.array([t for s in set_lists for t in s], np.int32)
    z_schur, status = ivcheck.host_z(corr[:, :p], set_off, sets, tx, ty, ts)
    assert not status.any()
    margin = float(np.min(np.abs(tz - tt)))
    dmax = float(np.max(np.abs(tz - z_schur)))
    marg, cond = ts < 0, ts >= 0
    verdict = tz < tt
    ok = margin >= 1000 * dmax
    for part in (marg, cond):
        ok = ok and part.any() and verdict[part].any() and (~verdict[part]).any()
    if p >= 3:
        ok = ok and all(0 < len(r) < len(cand) for r in rows.values())
    print(f"{name} seed {seed}: tests {tz.size} (marginal {int(marg.sum())}, conditional {int(cond.sum())}), sets {len(set_lists)}, "
          f"candidates {len(cand)}, rows {[len(r) for r in rows.values()]}, margin {margin:.3e}, d {dmax:.3e}, ok {ok}", flush=True)
    if not ok:
        return None
    arrays = dict(x=tx, y=ty, set=ts, alpha_id=ta, z=tz, thr=tt, set_off=set_off, sets=sets)
    arrays.update(candidates=np.array(cand, np.int32).reshape(-1, 3))
    for key, r in rows.items():
        arrays["rows_" + key] = np.array(r, np.int32).reshape(-1, 3)
    if inputs is not None:  # the files' text, byte for byte
        for key, txt in inputs.items():
            arrays["input_" + key] = np.frombuffer(txt.encode(), np.uint8)
    else:
        arrays.update(adj=adj.astype(np.int8), corr=corr)
    np.savez_compressed(os.path.join(HERE, f"iv_check_{name}.npz"), **arrays)
    return {"seed": seed, "traits": p, "markers": m, "noise": noise, "num_samples": N, "accept_alpha": a_acc,
            "reject_alpha": a_rej, "margin": margin, "d": dmax, "tests": int(tz.size), "input_as_text": as_text,
            "row_counts": {key: len(r) for key, r in rows.items()}, "candidate_count": len(cand)}

path = os.path.join(HERE, "iv_check_kat.json")
out = {"generator": "tests/golden/make_iv_check_golden.py", "cases": {}}
if ONLY and os.path.exists(path):
    out = json.load(open(path))
for name, seed, p, m, N, noise, a_acc, a_rej, flags, as_text in CASES:
    if ONLY and name not in ONLY.split(","):
        continue
    for attempt in range(40):
        got = run_case(name, seed + attempt, p, m, N, noise, a_acc, a_rej, flags, as_text)
        if got is not None:
            break
    assert got is not None, f"{name}: no seed satisfied the conditions"
    out["cases"][name] = got
with open(path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
