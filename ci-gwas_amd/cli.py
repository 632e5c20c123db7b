#!/usr/bin/env python3
"""`ci-gwas.py`-compatible command line for the cusk path on MI355X.

Mirrors the reference's workflow CLI for the two GPU subcommands
(/root/reference/ci-gwas.py:54-61 `prep-bed`, :63-92 `block`, :64-93 `cusk`, :95-253 `cuskss`, handlers :404-456): same
positional / optional arguments, same range checks, same conversion to the positional argv of
the native `mps` program with literal 'NULL' for absent paths, `subprocess.run(check=True)`.
`cuskss-het` and `cuskss-merged` (README.md:65,75 of the reference names them, its CLI does
not define them) are aliases of `cuskss` that insist on the flags that select that mode.
The workflow is prune-bed -> prep-bed -> prep-phen -> block -> cusk -> merge-block-outputs -> cuskss-merged -> sepselect ->
check-ivs -> mvivw.
`prune-bed` is not in the reference: its README asks for a fileset that is LD pruned ("or at least does not have markers
with a correlation of 1") and has no marker without recorded variation, and leaves both to the user.  Here they are
decided on the device, on the banded Kendall-npn correlation that `block` and the skeleton use (`mps prune`): markers in
.bim order per chromosome, the first kept marker wins.  That is not PLINK's rule (Pearson r^2, higher MAF kept).
`prep-phen` is not in the reference either: its README warns "make sure that the trait values are standardized" and its
loader takes the rows of the .phen as they come.  `prep-phen BFILES TABLE OUT [--covar FILE] [--ordinal NAMES]` matches a
trait table to the .fam by IID, removes the covariates from every trait by least squares (never from an ordinal one: a
residual has no levels) and standardises to mean 0 and population sd 1 over the observed values, on the device (`mps
prep-phen`; the rule is stated in include/cusk_hip.h).  `--rint [--rint-offset C]` then replaces every trait that is not
ordinal by the normal scores of its average ranks (cusk_phen_rint).  `check-phen BFILES PHEN` reports whether an existing .phen is
row-aligned and standardised and exits 1 if not.
Two more things the reference leaves to the user: `sumstats` writes the three correlation files of `cuskss` from a
PLINK set and a .phen, and `cuskss-merged --bfiles --phen` runs the merged step straight from those.  For phenotypes
with missing values `sumstats --se` adds the two standard-error files (from the number of individuals each pair was
observed on) and `cuskss-merged --bfiles --phen --het` tests every pair at that number.  `--ordinal NAMES` on either
marks binary or graded traits: their pairs get polychoric / polyserial correlations and standard errors.

`sepselect` and `orient-v-structs` (ci-gwas.py:303-358, handlers :467-476) run this package's device-backed
mirror of cusk_postprocessing/sepselect.py (ci-gwas_amd/sepselect.py) and write the same files.  With `--het` they
decide at the per-pair sample sizes a heterogeneous `cuskss-merged` run left in `cuskss_merged_ssz.mtx`.
`merge-block-outputs` (ci-gwas.py:255-271, :459-464) and the post-step of a merged `cuskss` run (:452-456) use this
package's mirror of the reference's merge module (ci-gwas_amd/merge.py), pinned by files the reference's own code
wrote (tests/golden/merge).  `iv-candidates` and `check-ivs` write the instrument tables of the reference's
cusk_postprocessing/check_mr_assumptions.py (`get_iv_candidates`, `check_ivs`; its CLI reaches them through `mvivw`) from a
merged skeleton, the tests of `check-ivs` on the device (ci-gwas_amd/ivcheck.py).  `mvivw` (ci-gwas.py:272-301, :479-503) writes the
candidate table and then the multivariable IVW estimates of every outcome, computed on the device (ci-gwas_amd/mvivw.py):
the plain IVW estimator with multiplicative random effects, NOT the reference's `mr_mvivw(..., robust = TRUE)`, which needs
R and robustbase::lmrob and can be neither run nor restated here.  The rest of the downstream (the R code of srfci) is the
reference's own code and consumes the files written here unchanged.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
MPS_PATH = os.environ.get("CUSK_MPS_PATH", os.path.join(_HERE, "csrc", "mps"))


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        sys.stderr.write(f"error: {message}\n")
        self.print_help()
        sys.exit(2)


class TypeCheck:
    """ci-gwas.py:27-40"""

    def __init__(self, type_fn, name, min_val=None, max_val=None):
        self._type_fn, self._name, self._min_val, self._max_val = type_fn, name, min_val, max_val

    def __call__(self, val):
        val = self._type_fn(val)
        if self._min_val is not None and val < self._min_val:
            raise argparse.ArgumentTypeError(f"Minimum {self._name} is {self._min_val}")
        if self._max_val is not None and val > self._max_val:
            raise argparse.ArgumentTypeError(f"Maximum {self._name} is {self._max_val}")
        return val


def _add_cusk(sub):
    p = sub.add_parser("cusk", help="Infer skeleton with markers and traits as nodes, using marker data (requires GPU)")
    p.add_argument("block_index", metavar="block-index", type=TypeCheck(int, "block-index", 0, None))
    p.add_argument("blocks", type=str, help="file with genomic block definitions (output of ci-gwas block)")
    p.add_argument("bfiles", type=str, help="filestem of .bed, .bim, .fam fileset")
    p.add_argument("phen", type=str, help="path to standardized phenotype tsv.")
    p.add_argument("alpha", type=TypeCheck(float, "alpha", 0.0, 1.0), default=10**-4)
    p.add_argument("max_level", metavar="max-level", type=TypeCheck(int, "max-level", 0, 14), default=3)
    p.add_argument("max_level_two", metavar="max-level-two", type=TypeCheck(int, "max-level", 0, 14), default=14)
    p.add_argument("max_depth", metavar="max-depth", type=TypeCheck(int, "max-depth", 1, None), default=1)
    p.add_argument("outdir", type=str, default="./")
    p.add_argument("--het", action="store_true",
                   help="test every marker-trait and trait-trait pair of the block at the number of individuals it was "
                        "observed on (phenotypes with NA entries), as `cuskss-merged --bfiles --phen --het` does afterwards")
    p.add_argument("--het-filter", action="store_true",
                   help="with --het: levels >= 2 of both stages through the filter and the recheck queue instead of the exact "
                        "path alone (`mps cusk ... het filter`); same output files")
    p.add_argument("--het-rows", action="store_true",
                   help="with --het: level 1 of both stages on the row-streaming kernel at per-pair sample sizes instead of the "
                        "exact sweep (`mps cusk ... het rows`); same output files")
    p.add_argument("--het-markers", action="store_true",
                   help="with --het: every pair of markers is tested at the number of individuals both were genotyped on "
                        "(.bed code 01 = missing) instead of all of them (`mps cusk ... het markers`); the output changes where "
                        "markers have missing calls")
    p.set_defaults(func=cusk)


def _add_prep(sub):
    """ci-gwas.py:54-61"""
    p = sub.add_parser("prep-bed", help="Prepare PLINK bed file for cusk")
    p.add_argument("bfiles", type=str, help="filestem of .bed, .bim, .fam fileset")
    p.set_defaults(func=prep_bed)


def _add_prune(sub):
    """not in ci-gwas.py: the reference's README asks for an LD-pruned fileset without constant markers and leaves it to
    the user"""
    p = sub.add_parser("prune-bed", help="Drop markers without recorded variation and LD-prune a PLINK fileset on the "
                                         "correlation the skeleton tests; goes in front of prep-bed (requires GPU)")
    p.add_argument("bfiles", type=str, help="filestem of .bed, .bim, .fam fileset")
    p.add_argument("out", type=str, help="filestem of the pruned fileset; also receives .prune.in and .prune.out")
    p.add_argument("--r-max", type=TypeCheck(float, "r-max", 0.0, 1.0), required=True,
                   help="drop a marker when |r| >= r-max with an earlier kept marker of its chromosome within the window "
                        "(banded Kendall-npn correlation, the one `block` and the skeleton use); in (0, 1].  The first kept "
                        "marker wins: not PLINK's rule, which keeps the marker with the higher MAF")
    p.add_argument("--window", type=TypeCheck(int, "window", 1, 4096), default=2000,
                   help="number of following markers each marker is compared with (default: the corr-width of block)")
    p.set_defaults(func=prune_bed)


def _add_prep_phen(sub):
    """not in ci-gwas.py: the reference's README leaves standardised traits to the user (cusk/scripts/phen_prep.py checks)"""
    p = sub.add_parser("prep-phen", help="Match a trait table to the .fam by IID, remove covariates from the traits and "
                                         "standardise them; goes in front of cusk / sumstats (requires GPU)")
    p.add_argument("bfiles", type=str, help="filestem of .bed, .bim, .fam fileset (the .fam is read)")
    p.add_argument("table", type=str, help="trait table: header FID IID <traits> (ids in either order, IID may be EID), NA = missing")
    p.add_argument("out", type=str, help="the .phen to write (one row per individual of the .fam, in its order); also "
                                         "receives <out>.prep.tsv with n, mean, sd and r2 per trait")
    p.add_argument("--covar", type=str, default=None, metavar="FILE",
                   help="covariate table in the format of the trait table (at most 63 numeric columns; dummy-code categories): "
                        "every trait is regressed on them, with an intercept, over the individuals that have the trait and "
                        "every covariate")
    p.add_argument("--ordinal", type=str, default=None, metavar="NAMES",
                   help="comma-separated names (or 1-based numbers) of the traits that are ordinal, as `sumstats --ordinal` "
                        "takes them: standardised only, never residualised (a residual has no levels)")
    p.add_argument("--rint", action="store_true",
                   help="rank-based inverse normal transform of every trait that is not ordinal, taken on the float32 "
                        "standardised residuals: average ranks for ties, normal scores of (rank - C) / (n + 1 - 2 C), "
                        "standardised again")
    p.add_argument("--rint-offset", type=float, default=None, metavar="C",
                   help="with --rint: the offset C in [0, 0.5] (default 0.375, Blom)")
    p.set_defaults(func=prep_phen)
    p = sub.add_parser("check-phen", help="Report whether a .phen is row-aligned to the .fam and standardised; exit status 1 "
                                          "if not (requires GPU)")
    p.add_argument("bfiles", type=str, help="filestem of .bed, .bim, .fam fileset (the .fam is read)")
    p.add_argument("phen", type=str, help="path to phenotype tsv")
    p.set_defaults(func=check_phen)


def _add_block(sub):
    """ci-gwas.py:63-92"""
    p = sub.add_parser("block", help="Tile whole-genome LD matrix into block diagonal matrix (requires GPU)")
    p.add_argument("bfiles", type=str, help="filestem of .bed, .bim, .fam fileset")
    p.add_argument("max_block_size", metavar="max-block-size", help="maximum number of markers per block", default=11000,
                   type=TypeCheck(int, "max-block-size", 2, None))
    p.add_argument("device_mem_gb", metavar="device-mem-gb", help="maximum memory available on GPU in GB", default=10,
                   type=TypeCheck(int, "device-mem-gb", 0, None))
    p.add_argument("corr_width", metavar="corr-width", help="width of banded-correlation matrix", default=2000,
                   type=TypeCheck(int, "corr-width", 2, None))
    p.set_defaults(func=block)


def _add_cuskss(sub, name, help_):
    p = sub.add_parser(name, help=help_)
    # cuskss-merged alone can take the genotypes instead of the three correlation files (cuskss_bed_argv): there --pxp
    # and --num-samples are asked for by cuskss_argv once it knows which route it is on
    from_bed = name == "cuskss-merged"
    p.add_argument("--mxm", type=str, default="NULL")
    p.add_argument("--mxp", type=str, default="NULL")
    p.add_argument("--pxp", type=str, required=not from_bed, default="NULL")
    p.add_argument("--mxp-se", type=str, default="NULL")
    p.add_argument("--pxp-se", type=str, default="NULL")
    p.add_argument("--block-index", metavar="block-index", type=TypeCheck(int, "block-index", 0, None), default=0)
    p.add_argument("--blockfile", type=str, default="NULL")
    p.add_argument("--marker-indices", metavar="marker-indices", type=str, default="NULL")
    p.add_argument("--alpha", type=TypeCheck(float, "alpha", 0.0, 1.0), required=True)
    p.add_argument("--max-level-one", metavar="max-level", type=TypeCheck(int, "max-level", 0, 14), default=3)
    p.add_argument("--max-level-two", metavar="max-level-two", type=TypeCheck(int, "max-level", 0, 14), default=14)
    p.add_argument("--max-depth", metavar="max-depth", type=TypeCheck(int, "max-depth", 1, None), default=1)
    p.add_argument("--time-index", type=str, default="NULL")
    p.add_argument("--num-samples", metavar="num-samples", type=TypeCheck(int, "num-samples", 1, None), required=not from_bed)
    p.add_argument("--outdir", type=str, default="./")
    if from_bed:
        p.add_argument("--bfiles", type=str, default=None,
                       help="filestem of .bed, .bim, .fam fileset (after prep-bed): compute the correlations from the "
                            "genotypes on the GPU instead of reading --mxm/--mxp/--pxp; needs --phen")
        p.add_argument("--phen", type=str, default=None, help="path to standardized phenotype tsv (with --bfiles)")
        p.add_argument("--het", action="store_true",
                       help="with --bfiles: per-pair sample sizes (the individuals both variables were observed on) instead "
                            "of the number of individuals; the result of --mxp-se/--pxp-se on the files of `sumstats --se`")
        p.add_argument("--het-markers", action="store_true",
                       help="with --bfiles and --het: also every pair of markers at the number of individuals both were "
                            "genotyped on instead of the number of individuals (`mps cuskss-bed ... het markers`)")
        p.add_argument("--ordinal", type=str, default=None, metavar="NAMES",
                       help="with --bfiles and --het: names (or 1-based numbers) of the ordinal traits, as `sumstats "
                            "--ordinal` takes them; the result of cuskss-het on the files it writes")
    p.set_defaults(func=cuskss, variant=name)


def _add_sumstats(sub):
    p = sub.add_parser("sumstats", help="Compute the correlation files of cuskss (mxm.bin, mxp.txt, pxp.txt) from "
                                        "genotypes and phenotypes (requires GPU)")
    p.add_argument("bfiles", type=str, help="filestem of .bed, .bim, .fam fileset (after prep-bed)")
    p.add_argument("phen", type=str, help="path to standardized phenotype tsv.")
    p.add_argument("outdir", type=str)
    p.add_argument("--marker-indices", metavar="marker-indices", type=str, default="NULL",
                   help="markers whose LD is written to mxm.bin (merged_blocks.ixs of merge-block-outputs); default: all")
    p.add_argument("--se", action="store_true",
                   help="also write mxp_se.txt and pxp_se.txt (for cuskss --mxp-se/--pxp-se): standard errors from the number "
                        "of individuals each pair was observed on, for a .phen with NA entries")
    p.add_argument("--ordinal", type=str, default=None, metavar="NAMES",
                   help="comma-separated names (or 1-based numbers) of the traits of the .phen that are ordinal (2 to 8 "
                        "distinct values, e.g. case/control): pairs with one of them get polychoric (marker or ordinal "
                        "partner) or polyserial (continuous partner) correlations and standard errors; implies --se")
    p.set_defaults(func=sumstats)


def _add_merge(sub):
    """ci-gwas.py:255-271"""
    p = sub.add_parser("merge-block-outputs", help="Merge outputs of cusk for all blocks into single files")
    p.add_argument("cusk_output_dir", metavar="cusk-output-dir", type=str, help="output directory of cusk")
    p.add_argument("blockfile", type=str, help="file with genomic block definitions (output of ci-gwas block)")
    p.set_defaults(func=merge_blocks)


def _add_sepselect(sub):
    """ci-gwas.py:303-358"""
    for name, help_, func in (
            ("orient-v-structs", "Orient v-structures using maximal separation sets on merged cusk skeletons.", run_v_struct),
            ("sepselect", "Compute maximal and partial-correlation-minimizing separation sets on merged cusk skeletons",
             run_sepselect)):
        p = sub.add_parser(name, help=help_)
        p.add_argument("cusk_result_stem", metavar="cusk-result-stem", type=str, help="outdir + stem of merged cusk results")
        p.add_argument("alpha", type=TypeCheck(float, "alpha", 0.0, 1.0), default=10**-4,
                       help="significance level for conditional independence tests")
        p.add_argument("num_samples", metavar="num-samples", type=TypeCheck(int, "num-samples", 1, None),
                       help="number of samples used for computing correlations")
        if name == "orient-v-structs":
            p.add_argument("--orientation-prior", metavar="orientation-prior", type=str, default=None,
                           help="matrix of (0, 1) (32 bit integers, binary) of dims (n_trait, n_trait) indicating "
                                "directions to be forced. ")
        p.add_argument("--het", action="store_true",
                       help="decide at the per-pair sample sizes of <cusk-result-stem>_ssz.mtx (written by cuskss-merged "
                            "--het) instead of num-samples, which is then not used")
        p.set_defaults(func=func)


def _add_ivcheck(sub):
    """the two tables of cusk_postprocessing/check_mr_assumptions.py"""
    p = sub.add_parser("iv-candidates", help="List the instrument candidates of every (exposure, outcome) pair of a merged "
                                             "skeleton")
    p.add_argument("cusk_output_stem", metavar="cusk-output-stem", type=str, help="outdir + stem of merged cusk results")
    p.set_defaults(func=run_iv_candidates)
    p = sub.add_parser("check-ivs", help="Filter instruments and exposures under the MR assumptions (requires GPU)")
    p.add_argument("cusk_output_stem", metavar="cusk-output-stem", type=str, help="outdir + stem of merged cusk results")
    p.add_argument("num_samples", metavar="num-samples", type=TypeCheck(int, "num-samples", 1, None),
                   help="number of samples used for computing correlations")
    p.add_argument("--accept-alpha", type=TypeCheck(float, "accept-alpha", 0.0, 1.0), required=True,
                   help="significance level at which a marginal dependence is accepted")
    p.add_argument("--reject-alpha", type=TypeCheck(float, "reject-alpha", 0.0, 1.0), required=True,
                   help="significance level of the conditional independence tests")
    p.add_argument("--relaxed-local-faithfulness", action="store_true",
                   help="do not ask for a marginal dependence of instrument and outcome")
    p.add_argument("--check-reverse-causality", action="store_true",
                   help="drop exposures that the outcome's own instruments point to as its effects")
    p.add_argument("--het", action="store_true",
                   help="decide at the per-pair sample sizes of <cusk-output-stem>_ssz.mtx (written by cuskss-merged --het) "
                        "instead of num-samples, which is then not used")
    p.add_argument("--out", type=str, default=None, help="output file (default <cusk-output-stem>_ivs.csv)")
    p.set_defaults(func=run_check_ivs)


def _add_mvivw(sub):
    """ci-gwas.py:272-301, with the selections of both of the reference's R scripts and the choices the R back-end fixes"""
    p = sub.add_parser("mvivw", help="Multivariable inverse-variance weighted Mendelian randomisation between the traits, "
                                     "using cusk-identified markers as instrumental variables: the plain IVW estimator with "
                                     "multiplicative random effects, or with --robust a stated M-estimator; neither is the "
                                     "reference's lmrob (requires GPU)")
    p.add_argument("cusk_output_stem", metavar="cusk-output-stem", type=str, help="output stem of cusk or cuskss result files")
    p.add_argument("num_samples", metavar="num-samples", type=TypeCheck(int, "num-samples", 1, None),
                   help="number of samples used for computing correlations")
    which = p.add_mutually_exclusive_group()
    which.add_argument("-s", action="store_true", help="use cusk inferred trait-trait skeleton to select exposures")
    which.add_argument("--orientation-prior", metavar="orientation-prior", type=str, default=None,
                       help="matrix of (0, 1) (32 bit integers, binary) of dims (n_trait, n_trait) indicating directions to be "
                            "forced. ")
    which.add_argument("--ivs", metavar="FILE", type=str, default=None,
                       help="table Exposure,Outcome,IV (as check-ivs writes it) that names the exposures and instruments of "
                            "every outcome")
    p.add_argument("--het", action="store_true",
                   help="weights from the per-pair sample sizes of <cusk-output-stem>_ssz.mtx (written by cuskss-merged --het) "
                        "instead of num-samples, which is then not used")
    p.add_argument("--model", choices=("default", "random", "fixed"), default="default",
                   help="standard errors: random = multiplicative random effects, fixed, default = random with four or more "
                        "instruments")
    p.add_argument("--ld", action="store_true",
                   help="treat the instruments of an outcome as correlated: generalised least squares with the marker block of "
                        "<cusk-output-stem>_scm.mtx as their LD; <stem>_mvivw_outcomes.tsv gains the column ld_pivot")
    p.add_argument("--ld-ridge", metavar="L", type=TypeCheck(float, "ld-ridge", 0.0, None), default=None,
                   help="with --ld: shrink the LD towards the identity, (1 - L) R + L I, 0 <= L < 1 (default 0)")
    p.add_argument("--robust", nargs="?", const="bisquare", default=None, choices=("huber", "bisquare"),
                   help="outlier-resistant estimates by iteratively reweighted least squares: huber, or bisquare (Huber, "
                        "then Tukey bisquare weights; the default of a bare --robust).  A stated, deterministic M-estimator, "
                        "not the reference's lmrob.  <stem>_mvivw_outcomes.tsv gains the columns scale tau iterations rho_sum")
    p.add_argument("--robust-weights", metavar="FILE", type=str, default=None,
                   help="with --robust: write sink, marker, rho of every instrument whose final weight rho is below 1")
    jk = p.add_mutually_exclusive_group()
    jk.add_argument("--jackknife", metavar="loo|B", type=str, default=None,
                    help="refit every outcome without each group of its instruments: loo = one group per instrument (the "
                         "leave-one-out table and PRESS), B >= 2 = that many contiguous groups of the instrument list (the "
                         "delete-one-block jackknife, whose standard error needs no LD matrix).  <stem>_mvivw_results.tsv gains "
                         "the columns jk_effect jk_se jk_p jk_min jk_max jk_marker, <stem>_mvivw_outcomes.tsv jk_groups press "
                         "jk_pivot jk_status.  Not MR-PRESSO: no simulated null, no p-value of the global test")
    jk.add_argument("--jackknife-groups", metavar="FILE", type=str, default=None,
                    help="the same with groups from FILE: one non-decreasing integer label per marker row (LD blocks); a "
                         "group is a run of instruments with one label")
    p.add_argument("--jackknife-residuals", metavar="FILE", type=str, default=None,
                   help="with --jackknife / --jackknife-groups: write sink, marker, group, press_residual of every instrument")
    p.add_argument("--jackknife-table", metavar="FILE", type=str, default=None,
                   help="with --jackknife / --jackknife-groups: write the estimates without each group")
    p.add_argument("--out", type=str, default=None, help="output file (default <cusk-output-stem>_mvivw_results.tsv)")
    p.set_defaults(func=run_mvivw, parser=p)


def build_parser() -> argparse.ArgumentParser:
    parser = _Parser(prog="ci-gwas", description="cusk / cuskss steps of CI-GWAS on AMD Instinct MI355X")
    sub = parser.add_subparsers(required=True, title="subcommands")
    _add_prune(sub)
    _add_prep(sub)
    _add_prep_phen(sub)
    _add_block(sub)
    _add_cusk(sub)
    _add_cuskss(sub, "cuskss", "Infer skeleton using summary statistic data (requires GPU)")
    _add_cuskss(sub, "cuskss-het", "cuskss with heterogeneous (polychoric/polyserial) correlations: needs --mxp-se/--pxp-se")
    _add_cuskss(sub, "cuskss-merged", "cuskss on the union of markers selected in all blocks: needs --marker-indices")
    _add_sumstats(sub)
    _add_merge(sub)
    _add_sepselect(sub)
    _add_ivcheck(sub)
    _add_mvivw(sub)
    return parser


def prep_bed(args):
    """ci-gwas.py:386-387"""
    subprocess.run([MPS_PATH, "prep", args.bfiles], check=True)


def prune_argv(args) -> list[str]:
    """`mps prune <bfiles> <out-stem> <r-max> <window>`"""
    if args.r_max == 0:
        sys.exit("prune-bed: --r-max 0 would drop every marker that has a neighbour: give a value in (0, 1].")
    if args.out == args.bfiles or any(os.path.exists(args.out + sfx) and os.path.exists(args.bfiles + sfx)
                                      and os.path.samefile(args.out + sfx, args.bfiles + sfx) for sfx in (".bed", ".bim", ".fam")):
        sys.exit("prune-bed: the output stem must differ from bfiles.")
    return [MPS_PATH, "prune", args.bfiles, args.out, repr(float(args.r_max)), str(args.window)]


def prune_bed(args):
    subprocess.run(prune_argv(args), check=True)


def block_argv(args) -> list[str]:
    """ci-gwas.py `block` handler"""
    return [MPS_PATH, "block", args.bfiles, str(args.max_block_size), str(args.device_mem_gb), str(args.corr_width)]


def block(args):
    subprocess.run(block_argv(args), check=True)


def cusk_argv(args) -> list[str]:
    """ci-gwas.py:404-420"""
    if getattr(args, "het_filter", False) and not getattr(args, "het", False):
        sys.exit("cusk: --het-filter applies to runs at per-pair sample sizes: give --het with it.")
    if getattr(args, "het_rows", False) and not getattr(args, "het", False):
        sys.exit("cusk: --het-rows applies to runs at per-pair sample sizes: give --het with it.")
    if getattr(args, "het_markers", False) and not getattr(args, "het", False):
        sys.exit("cusk: --het-markers applies to runs at per-pair sample sizes: give --het with it.")
    return [MPS_PATH, "cusk", args.phen, args.bfiles, args.blocks, str(args.alpha), str(args.max_level),
            str(args.max_level_two), str(args.max_depth), args.outdir, str(args.block_index)] + (
                ["het"] if getattr(args, "het", False) else []) + (["filter"] if getattr(args, "het_filter", False) else []) + (
                    ["rows"] if getattr(args, "het_rows", False) else []) + (
                        ["markers"] if getattr(args, "het_markers", False) else [])


NA_TOKENS = ("NA", "NaN", "nan", "NAN")  # is_na_token of csrc/host/host_io.h


def ordinal_arg(command: str, names: str, phen_path: str) -> str:
    """`--ordinal NAMES` -> `ordinal=<1-based,...>` of the native program: names are looked up in the header of the .phen
    (two id columns, then the traits), numbers are taken as they are; every named trait must have 2 to 8 distinct
    non-NA values.  `mps` checks the levels again on the table it loads; here the file is streamed once and only the
    named columns are looked at, so that a wrong name or a continuous trait is an argument error before the GPU is asked
    for."""
    try:
        f = open(phen_path)
    except OSError:
        sys.exit(f"{command}: cannot read {phen_path}.")
    with f:
        traits = f.readline().split()[2:]
        numbers = []
        for tok in names.split(","):
            tok = tok.strip()
            if tok in traits:
                num = traits.index(tok) + 1
            elif tok.isdigit():
                num = int(tok)
                if not 1 <= num <= len(traits):
                    sys.exit(f"{command}: --ordinal trait number {num} is out of range (1 .. {len(traits)}).")
            else:
                sys.exit(f"{command}: --ordinal names an unknown trait '{tok}' (the .phen has: {' '.join(traits)}).")
            if num in numbers:
                sys.exit(f"{command}: --ordinal names trait '{tok}' twice.")
            numbers.append(num)
        limit = 4096  # enough to tell a graded trait from a continuous one without keeping all of the latter
        distinct = {num: set() for num in numbers}
        for line in f:
            w = line.split()
            for num, seen in distinct.items():
                if len(seen) > limit or num + 1 >= len(w) or w[num + 1] in NA_TOKENS:
                    continue
                try:
                    x = float(w[num + 1])
                except ValueError:
                    sys.exit(f"{command}: cannot read the value '{w[num + 1]}' of trait {traits[num - 1]}.")
                if x == x:
                    seen.add(x)
    for num in numbers:
        count = len(distinct[num])
        shown = f"more than {limit}" if count > limit else str(count)
        if count > 8:
            sys.exit(f"{command}: --ordinal trait {traits[num - 1]} has {shown} distinct values; at most 8 levels are "
                     "supported.")
        if count < 2:
            sys.exit(f"{command}: --ordinal trait {traits[num - 1]} has {shown} distinct values; at least 2 levels are "
                     "needed.")
    return "ordinal=" + ",".join(str(v) for v in numbers)


def sumstats_argv(args) -> list[str]:
    ordinal = getattr(args, "ordinal", None)
    tail = ["se", ordinal_arg("sumstats", ordinal, args.phen)] if ordinal is not None else (["se"] if args.se else [])
    return [MPS_PATH, "sumstats", args.phen, args.bfiles, args.marker_indices, args.outdir] + tail


def sumstats(args):
    subprocess.run(sumstats_argv(args), check=True)


def _same_path(a: str, b: str) -> bool:
    return a == b or (os.path.exists(a) and os.path.exists(b) and os.path.samefile(a, b))


def prep_phen_argv(args) -> list[str]:
    """`mps prep-phen <bfiles> <table> <out> <covar|NULL> [ordinal=<1-based,...>] [rint|rint=<offset>]`"""
    covar = getattr(args, "covar", None)
    rint, offset = getattr(args, "rint", False), getattr(args, "rint_offset", None)
    if offset is not None and not rint:
        sys.exit("prep-phen: --rint-offset needs --rint.")
    if offset is not None and not 0.0 <= offset <= 0.5:  # false for NaN too
        sys.exit(f"prep-phen: --rint-offset {offset} is not in [0, 0.5].")
    if _same_path(args.out, args.table):
        sys.exit("prep-phen: OUT must differ from TABLE.")
    if covar is not None and _same_path(args.out, covar):
        sys.exit("prep-phen: OUT must differ from the --covar file.")
    if _same_path(args.out, args.bfiles + ".fam"):
        sys.exit("prep-phen: OUT must differ from the .fam.")
    ordinal = getattr(args, "ordinal", None)
    return [MPS_PATH, "prep-phen", args.bfiles, args.table, args.out, covar if covar is not None else "NULL"] + (
        [ordinal_arg("prep-phen", ordinal, args.table)] if ordinal is not None else []) + (
        ["rint" if offset is None else f"rint={offset!r}"] if rint else [])


def check_phen_argv(args) -> list[str]:
    """`mps check-phen <bfiles> <phen>`"""
    return [MPS_PATH, "check-phen", args.bfiles, args.phen]


def prep_phen(args):
    subprocess.run(prep_phen_argv(args), check=True)


def check_phen(args):
    """exit status 1 (and one line per failing trait on stdout) when the .phen is not row-aligned and standardised"""
    sys.exit(subprocess.run(check_phen_argv(args)).returncode)


def cuskss_bed_argv(args) -> list[str]:
    """`cuskss-merged --bfiles STEM --phen FILE`: the correlations of the selected markers and the traits are computed
    from the genotypes and swept without leaving the GPU (`mps cuskss-bed`); same result files as the file route on
    what `sumstats` writes"""
    if args.bfiles is None or args.phen is None:
        sys.exit("cuskss-merged: --bfiles and --phen go together.")
    if getattr(args, "het_markers", False) and not args.het:
        sys.exit("cuskss-merged: --het-markers applies to runs at per-pair sample sizes: give --het with it.")
    if getattr(args, "ordinal", None) is not None and not args.het:
        sys.exit("cuskss-merged: --ordinal estimates come with their own standard errors: give --het with it.")
    if any(v != "NULL" for v in (args.mxm, args.mxp, args.pxp)):
        sys.exit("cuskss-merged: give either --bfiles/--phen or --mxm/--mxp/--pxp, not both.")
    if args.mxp_se != "NULL" or args.pxp_se != "NULL":
        sys.exit("cuskss-merged: --mxp-se/--pxp-se cannot be combined with --bfiles (Pearson correlations have no "
                 "standard-error files).")
    if args.blockfile != "NULL":
        sys.exit("cuskss-merged: --blockfile does not apply with --bfiles.")
    if args.marker_indices == "NULL":
        sys.exit("cuskss-merged needs --marker-indices.")
    if args.num_samples is not None:
        try:
            with open(args.bfiles + ".dim") as f:
                in_dim = int(f.readline().split()[0])
        except (OSError, ValueError, IndexError):
            sys.exit(f"cuskss-merged: cannot read {args.bfiles}.dim (run prep-bed first).")
        if in_dim != args.num_samples:
            sys.exit(f"cuskss-merged: --num-samples {args.num_samples} differs from the {in_dim} individuals of "
                     f"{args.bfiles}.dim.")
    return [MPS_PATH, "cuskss-bed", args.phen, args.bfiles, args.marker_indices, args.time_index, str(args.alpha),
            str(args.max_level_one), str(args.max_level_two), str(args.max_depth), args.outdir] + (["het"] if args.het else []) + (
                ["markers"] if getattr(args, "het_markers", False) else []) + (
                    [ordinal_arg("cuskss-merged", args.ordinal, args.phen)] if getattr(args, "ordinal", None) is not None else [])


def cuskss_argv(args) -> list[str]:
    """ci-gwas.py:423-451 (validation :424-429 included)"""
    if getattr(args, "bfiles", None) is not None or getattr(args, "phen", None) is not None:
        return cuskss_bed_argv(args)
    if getattr(args, "het", False):
        sys.exit("cuskss-merged: --het needs --bfiles and --phen (with correlation files, give --mxp-se/--pxp-se).")
    if getattr(args, "het_markers", False):
        sys.exit("cuskss-merged: --het-markers needs --bfiles, --phen and --het (correlation files carry no marker x marker sizes).")
    if getattr(args, "ordinal", None) is not None:
        sys.exit("cuskss-merged: --ordinal needs --bfiles, --phen and --het (correlation files already hold their estimates).")
    if args.pxp == "NULL":
        sys.exit("the following arguments are required: --pxp")
    if args.num_samples is None:
        sys.exit("the following arguments are required: --num-samples")
    if args.blockfile == "NULL" and args.marker_indices == "NULL":
        sys.exit("Either blockfile + block index or marker indices into the mxp file have to be provided for cuskss.")
    if sum([args.mxp_se == "NULL", args.pxp_se == "NULL"]) == 1:
        sys.exit("Please provide no or both pxp and mxp standard error files.")
    if sum([args.mxp == "NULL", args.mxm == "NULL"]) == 1:
        sys.exit("Please provide no or both mxp and mxm correlation files.")
    variant = getattr(args, "variant", "cuskss")
    if variant == "cuskss-het" and args.mxp_se == "NULL":
        sys.exit("cuskss-het needs --mxp-se and --pxp-se.")
    if variant == "cuskss-merged" and args.marker_indices == "NULL":
        sys.exit("cuskss-merged needs --marker-indices.")
    return [MPS_PATH, "cuskss", args.mxm, args.mxp, args.mxp_se, args.pxp, args.pxp_se, args.time_index,
            str(args.block_index), args.blockfile, args.marker_indices, str(args.alpha), str(args.max_level_one),
            str(args.max_level_two), str(args.max_depth), str(args.num_samples), args.outdir]


def cusk(args):
    subprocess.run(cusk_argv(args), check=True)


def cuskss(args):
    subprocess.run(cuskss_argv(args), check=True)
    if args.marker_indices != "NULL":
        # ci-gwas.py:452-456: the merged output is rewritten into the sparse merge format (needs
        # <outdir>/merged_blocks.ixs, as in the reference)
        from .merge import reformat_cuskss_merged_output

        reformat_cuskss_merged_output(cusk_dir=args.outdir).write_mm(basepath=f"{args.outdir}/cuskss_merged")


def merge_blocks(args):
    """ci-gwas.py:459-464"""
    from .merge import merge_block_outputs

    out_dir = args.cusk_output_dir if args.cusk_output_dir.endswith("/") else args.cusk_output_dir + "/"
    merge_block_outputs(args.blockfile, out_dir).write_mm(f"{args.cusk_output_dir}/merged_blocks")


def run_sepselect(args):
    """ci-gwas.py:467-470"""
    from .sepselect import sepselect_merged

    merged_cusk = sepselect_merged(args.cusk_result_stem, args.alpha, args.num_samples, het=args.het)
    merged_cusk.to_file(f"{os.path.dirname(args.cusk_result_stem)}/max_sep_min_pc")
    print("Sepselect done.")


def run_v_struct(args):
    """ci-gwas.py:473-476"""
    from .sepselect import orient_v_structures_merged

    merged_cusk = orient_v_structures_merged(args.cusk_result_stem, args.alpha, args.num_samples, args.orientation_prior,
                                             het=args.het)
    merged_cusk.to_file(f"{os.path.dirname(args.cusk_result_stem)}/max_sep_min_pc")
    print("Sepselect / v-structs done.")


def run_iv_candidates(args):
    from .ivcheck import iv_candidates, write_csv

    write_csv(f"{args.cusk_output_stem}_iv_candidates.csv", iv_candidates(args.cusk_output_stem))


def run_check_ivs(args):
    from .ivcheck import check_ivs, load, write_csv

    data = load(args.cusk_output_stem, het=args.het)  # unreadable inputs are reported before an engine exists; read once
    from .skeleton import Engine

    rows = check_ivs(args.cusk_output_stem, args.num_samples, args.accept_alpha, args.reject_alpha,
                     relaxed_local_faithfulness=args.relaxed_local_faithfulness,
                     check_reverse_causality=args.check_reverse_causality, het=args.het, engine=Engine(0), data=data)
    write_csv(args.out or f"{args.cusk_output_stem}_ivs.csv", rows)
    print(f"check-ivs: {len(rows)} instrument rows.")


def _mvivw_engine():
    from .skeleton import Engine

    return Engine(0)


def run_mvivw(args):
    """ci-gwas.py:479-503: the candidate table first, then the estimates (here on the device instead of in R)"""
    from . import mvivw
    from .ivcheck import iv_candidates, load, write_csv

    stem = args.cusk_output_stem
    if args.ld_ridge is not None and not args.ld:
        args.parser.error("--ld-ridge needs --ld")
    if args.ld_ridge is not None and not args.ld_ridge < 1.0:
        args.parser.error("--ld-ridge must be in [0, 1)")
    if args.robust and args.ld:
        args.parser.error("--robust cannot be combined with --ld: whitening mixes the rows, so a weight per instrument "
                          "has no meaning there")
    if args.robust_weights and not args.robust:
        args.parser.error("--robust-weights needs --robust")
    with_jk = args.jackknife is not None or args.jackknife_groups is not None
    if with_jk and (args.ld or args.robust):
        args.parser.error("--jackknife cannot be combined with --ld or --robust: whitening mixes the rows, and a reweighted "
                          "refit per deletion is another estimator")
    if (args.jackknife_residuals or args.jackknife_table) and not with_jk:
        args.parser.error("--jackknife-residuals and --jackknife-table need --jackknife or --jackknife-groups")
    jackknife = None
    if args.jackknife is not None:
        if args.jackknife != "loo" and not (args.jackknife.isdigit() and int(args.jackknife) >= 2):
            args.parser.error("--jackknife takes loo or a number of groups >= 2")
        jackknife = "loo" if args.jackknife == "loo" else int(args.jackknife)
    data = load(stem, het=args.het)  # unreadable inputs are reported before an engine exists; read once
    if args.jackknife_groups is not None:
        jackknife = mvivw.read_group_labels(args.jackknife_groups, data[0].shape[0] - data[2])
    write_csv(f"{stem}_iv_candidates.csv", iv_candidates(stem, data=data))
    mode = "skeleton" if args.s else "prior" if args.orientation_prior else "ivs" if args.ivs else "all"
    res = mvivw.run(stem, args.num_samples, mode=mode, prior_path=args.orientation_prior, ivs_path=args.ivs, het=args.het,
                    model=mvivw.MODELS[args.model], engine=_mvivw_engine(), data=data, ld=args.ld, ld_ridge=args.ld_ridge or 0.0,
                    robust=args.robust, jackknife=jackknife)
    out = args.out or f"{stem}_mvivw_results.tsv"
    mvivw.write_results(out, res)
    mvivw.write_outcomes(f"{out[:-len('_results.tsv')]}_outcomes.tsv" if out.endswith("_results.tsv") else f"{out}.outcomes.tsv", res)
    if args.robust_weights:
        mvivw.write_weights(args.robust_weights, res)
    if args.jackknife_residuals:
        mvivw.write_jackknife_residuals(args.jackknife_residuals, res)
    if args.jackknife_table:
        mvivw.write_jackknife_table(args.jackknife_table, res)
    print(f"mvivw: {int((res['status'] == 0).sum())} of {res['p']} outcomes estimated.")


def main(argv=None):
    args = build_parser().parse_args(argv)
    args.func(args)


if __name__ == "__main__":
    main()
