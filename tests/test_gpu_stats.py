"""The device sampler of the statistical stage (csrc/mdx_stats.hip) against the numpy restatement of the reference's R
model (tests/stats_model.py), and the command line around it."""

import functools
import math
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import stats_cases as C  # noqa: E402
import stats_model as M  # noqa: E402
from mapdamage_amd import stats  # noqa: E402

pytestmark = pytest.mark.gpu
M24 = 24


def options(termini="both", **kw):
    kw.setdefault("fix_nicks", True)
    kw.setdefault("seq_length", M24 // 2 if termini == "both" else M24)
    return stats.StatsOptions(termini=termini, **kw)


# ---------------------------------------------------------------------- the log-likelihood
@functools.lru_cache(maxsize=None)
def loglik_tables(termini):
    """Counts of about 10 and about 10^6 a cell row, and a table with empty cells (3 bases a row)."""
    tables = [C.model_table(M24, termini, n, 40 + i, diff_hangs=False) for i, n in enumerate((10, 1_000_000, 3))]
    assert (tables[2] == 0).sum() > 100
    return np.stack(tables)


def start_like_vectors(rng, n):
    """The distributions of start.r:60-66, LambdaDisp from its values up to 4: the bound below covers the summation and the
    logarithms, and with a dispersion of 50 or more the lgamma terms of dnbinom (about 2000, one ulp 2e-13) cancel to
    leave two correct implementations a relative 1e-13 apart in the overhang vector before any term is summed."""
    x = rng.uniform(size=(n, 7))
    x[:, M.DISP] = rng.choice(M.DISP_STARTS[:5], n)
    x[:, M.RHO] = rng.choice(M.RHO_STARTS, n)
    return x


@pytest.mark.parametrize("jukes_cantor", [False, True], ids=["hky", "jc"])
@pytest.mark.parametrize("termini", ["both", "5p", "3p"])
def test_loglik_matches_the_restatement(termini, jukes_cantor):
    tables = loglik_tables(termini)
    nu = C.fixed_nu(M24, termini)
    opts = options(termini, jukes_cantor=jukes_cantor, diff_hangs=termini == "both", var_disp=True)
    mopts = M.Options(M24, termini, jukes_cantor, termini == "both", True)
    x = start_like_vectors(np.random.default_rng(17), 200)
    params, table_of = np.repeat(x, 3, axis=0), np.tile(np.arange(3, dtype=np.int32), 200)
    got = stats.loglik(tables, nu, C.ACGT, table_of, params, opts)
    consts = [M.lnfact_constant(t) for t in tables]
    worst = 0.0
    for e in range(len(params)):
        want, total = M.loglik_of(tables[table_of[e]], consts[table_of[e]], nu, C.ACGT, mopts, params[e], with_abs=True)
        assert math.isfinite(want)
        bound = 512 * 2.0 ** -53 * total
        worst = max(worst, abs(got[e] - want) / bound)
        assert abs(got[e] - want) <= bound, (e, got[e], want, bound)
    print("worst |delta| / bound: %.3f" % worst)


def test_loglik_out_of_range_is_minus_infinity():
    tables = loglik_tables("both")
    nu = C.fixed_nu(M24, "both")
    good = np.array(C.TRUTH)
    bad = []
    for index, value in ((M.THETA, -1e-9), (M.RHO, 0.0), (M.RHO, -1.0), (M.DELTAD, -0.1), (M.DELTAD, 1.5), (M.DELTAS, -1e-12),
                         (M.DELTAS, 1.0000001), (M.LAMBDA, -0.2), (M.LAMBDA, 1.2), (M.LAMBDAR, 1.01), (M.DISP, -3.0),
                         (M.DELTAD, math.nan)):
        v = good.copy()
        v[index] = value
        bad.append(v)
    params = np.stack([good] + bad)
    got = stats.loglik(tables, nu, C.ACGT, np.zeros(len(params), np.int32), params, options(diff_hangs=True, var_disp=True))
    assert math.isfinite(got[0])
    assert (got[1:] == -math.inf).all(), got


# ---------------------------------------------------------------------- the substitution matrix
def test_hky_closed_form_against_eig():
    rng = np.random.default_rng(23)
    n = 300
    acgt = rng.uniform(0.1, 0.4, size=(n, 4))
    acgt /= acgt.sum(axis=1, keepdims=True)
    acgt = np.clip(acgt, 0.1, 0.4)
    acgt /= acgt.sum(axis=1, keepdims=True)
    rho, tmu = rng.uniform(0.3, 3, n), 10 ** rng.uniform(-4, math.log10(2), n)
    got = stats.substitution_matrices(np.column_stack([tmu, rho, acgt]))
    for k in range(n):
        np.testing.assert_allclose(got[k], M.pmat(tmu[k], rho[k], acgt[k]), rtol=0, atol=1e-10)
    assert np.abs(got.sum(axis=2) - 1).max() <= 1e-13
    jc = stats.substitution_matrices(np.column_stack([tmu, rho, acgt]), jukes_cantor=True)
    for k in range(0, n, 30):
        np.testing.assert_allclose(jc[k], M.pmat(tmu[k], 1.0, [0.25] * 4, True), rtol=1e-15, atol=0)


# ---------------------------------------------------------------------- a chain against its restatement
def parity_options(name, **kw):
    m, termini, flags, seed, _ = C.PARITY[name]
    r = C.PARITY_RUN
    return stats.StatsOptions(seq_length=m // 2 if termini == "both" else m, termini=termini, rand=r["n_rand"], burn=r["n_burn"],
                              adjust=r["n_adjust"], iterations=r["n_iter"], fix_nicks=True, seed=seed, n_pred=2000, **flags, **kw)


@functools.lru_cache(maxsize=None)
def parity_device(name):
    table, nu, _, _, chain_id = C.parity_inputs(name)
    return stats.run_chains(table[None], nu, C.ACGT, parity_options(name), [chain_id])[0]


@pytest.mark.parametrize("name", ["full", "m2", "5p"])
def test_chain_follows_the_restatement(name):
    chain, want = C.parity_restatement(name)
    assert chain.margin > 1e-6, chain.margin            # no accept decision of the run is within rounding of its threshold
    got = parity_device(name)
    np.testing.assert_allclose(got.start[:7], chain.start, rtol=1e-12)
    np.testing.assert_allclose(got.trace, want, rtol=1e-9)
    np.testing.assert_allclose(got.prop_sd, chain.sd, rtol=0, atol=0)
    np.testing.assert_allclose(got.acc, [M.acc_rat(want[:, q]) for q in range(8)], rtol=1e-15)


@pytest.mark.parametrize("name", ["full", "5p"])
def test_correcting_probabilities(name):
    """From the device's own trace and the same draws."""
    table, nu, mopts, seed, chain_id = C.parity_inputs(name)
    got = parity_device(name)
    rounds = max(C.PARITY_RUN["n_adjust"], 1)
    want = M.correcting(got.trace, nu, C.ACGT, mopts, seed, chain_id, 2 + rounds, 2000)
    np.testing.assert_allclose(got.corr, want, rtol=1e-9)
    assert (got.corr >= 0).all() and (got.corr <= 1).all()


# ---------------------------------------------------------------------- isolation and determinism
def test_a_chain_does_not_depend_on_its_launch():
    opts = stats.StatsOptions(rand=3, burn=40, adjust=2, iterations=80, fix_nicks=True, diff_hangs=True, var_disp=True, seed=5, n_pred=100)
    nu = C.fixed_nu(M24, "both")
    tables = np.stack([C.model_table(M24, "both", 500 + 10 * k, 300 + k) for k in range(70)])
    ids = np.arange(70, dtype=np.uint32) + 100

    def run(members, seed_options=opts):
        out = stats.run_chains(tables[members], nu, C.ACGT, seed_options, ids[members])
        return out[list(members).index(6)]

    alone, nine, seventy, again = run([6]), run(list(range(9))), run(list(range(70))), run([6])
    for other in (nine, seventy, again):
        for field in ("trace", "prop_sd", "acc", "corr", "start"):
            assert getattr(alone, field).tobytes() == getattr(other, field).tobytes(), field
    assert len(np.unique(alone.trace[:, M.DELTAS])) > 5
    other_seed = stats.StatsOptions(rand=3, burn=40, adjust=2, iterations=80, fix_nicks=True, diff_hangs=True, var_disp=True, seed=6, n_pred=100)
    assert run([6], other_seed).trace.tobytes() != alone.trace.tobytes()
    # (and the chain id is part of the key)
    assert stats.run_chains(tables[[6]], nu, C.ACGT, opts, [7])[0].trace.tobytes() != alone.trace.tobytes()


# ---------------------------------------------------------------------- recovery
def test_default_chain_recovers_the_parameters():
    """2 (l(MLE) - l(truth)) is chi-squared with at most 7 degrees of freedom, P(chi2 > 40) < 1e-5; the posterior mean lies
    within that of the maximum."""
    truth = (0.012, 1.3, 0.02, 0.6, 0.35, 0.35, 1.0)
    mopts = M.Options(M24, "both")
    nu = C.fixed_nu(M24, "both")
    table = M.simulate_table(np.random.default_rng(77), mopts, C.ACGT, nu, truth, 1_000_000)
    got = stats.run_chains(table[None], nu, C.ACGT, stats.StatsOptions(fix_nicks=True, seed=2024))[0]
    assert got.trace.shape == (50000, 8)
    mean = got.trace[:, :7].mean(axis=0)
    const = M.lnfact_constant(table)
    at_mean, at_truth = (M.loglik_of(table, const, nu, C.ACGT, mopts, x) for x in (mean, truth))
    print("l(mean) %.3f  l(truth) %.3f  mean %s" % (at_mean, at_truth, mean))
    assert at_mean >= at_truth - 20


# ---------------------------------------------------------------------- the command line
RGS = [{"ID": "rg1", "SM": "s1", "LB": "lib1"}]
FAST = ["--fix-nicks", "--rand", "4", "--adjust", "2", "--burn", "100", "--iter", "200", "--stats-seed", "9"]
CSVS = (stats.ITER_CSV, stats.SUMM_CSV, stats.CORR_CSV)


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    from mapdamage_amd import fasta, sam, synth
    d = tmp_path_factory.mktemp("stats_cli")
    ref = synth.make_genome(seed=61, sizes=(("chrA", 6000), ("chrB", 4000), ("chrC", 3000)), n_run=40, lower_run=200)
    batch = synth.make_reads(ref, 9000, 62, read_len=60, with_qual=True)
    fasta.write_fasta(d / "ref.fa", ref)
    sam.write_bam(str(d / "in.bam"), batch, ref.names, ref.lengths, RGS, ["rg1"] * batch.n)
    for g in range(3):
        part = batch.take(np.flatnonzero(np.asarray(batch.tid) == g))
        assert part.n > 1000
        sam.write_bam(str(d / ("only%d.bam" % g)), part, ref.names, ref.lengths, RGS, ["rg1"] * part.n)
    return d


def test_rescale_in_one_run(cli_files, tmp_path):
    from mapdamage_amd.main import main
    from mapdamage_amd.rescale import RescaleModel
    d, out = cli_files, tmp_path / "out"
    assert main(["-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(out), "--rescale"] + FAST) == 0
    for name in CSVS + ("dnacomp_genome.csv", "misincorporation.txt"):
        assert (out / name).is_file(), name
    assert len((out / stats.ITER_CSV).read_text().splitlines()) == 201
    model = RescaleModel.from_csv(out / stats.CORR_CSV, 12, 12)
    assert len(model.corr_prob) == 48 and all(0 <= v <= 1 for v in model.corr_prob.values())
    assert model.corr_prob[("C", "T", 1)] > model.corr_prob[("C", "T", 12)]          # the synthetic damage decays inwards
    rescaled = (out / "in.rescaled.bam").read_bytes()
    again = tmp_path / "again.bam"
    assert main(["-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(out), "--rescale-only", "--rescale-out", str(again)]) == 0
    assert again.read_bytes() == rescaled and len(rescaled) > 10000
    # --stats-only from the folder: the same three files
    before = {name: (out / name).read_bytes() for name in CSVS}
    for name in CSVS:
        (out / name).unlink()
    assert main(["-d", str(out), "--stats-only"] + FAST) == 0
    assert {name: (out / name).read_bytes() for name in CSVS} == before


def test_stats_by_reference(cli_files, tmp_path):
    from mapdamage_amd.main import main
    d, out = cli_files, tmp_path / "out"
    assert main(["-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(out), "--stats", "--by-reference"] + FAST) == 0
    for g in range(3):
        alone = tmp_path / ("alone%d" % g)
        assert main(["-i", str(d / ("only%d.bam" % g)), "-r", str(d / "ref.fa"), "-d", str(alone), "--stats",
                     "--stats-chain", str(g + 1)] + FAST) == 0
        for name in CSVS:
            assert (out / "by_reference" / str(g) / name).read_bytes() == (alone / name).read_bytes(), (g, name)
    assert (out / stats.CORR_CSV).read_bytes() != (out / "by_reference" / "0" / stats.CORR_CSV).read_bytes()
