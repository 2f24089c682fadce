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


def options(termini="both", m=M24, **kw):
    kw.setdefault("fix_nicks", True)
    kw.setdefault("seq_length", m // 2 if termini == "both" else m)
    return stats.StatsOptions(termini=termini, **kw)


# ---------------------------------------------------------------------- the log-likelihood
@functools.lru_cache(maxsize=None)
def loglik_tables(termini, m=M24, nu_kind="fixed"):
    """Counts of about 10 and about 10^6 a cell row, and a table with empty cells (3 bases a row)."""
    tables = [C.model_table(m, termini, n, 40 + i, diff_hangs=False, nu_kind=nu_kind) for i, n in enumerate((10, 1_000_000, 3))]
    assert (tables[2] == 0).sum() > 100
    return np.stack(tables)


def start_like_vectors(rng, n):
    """The distributions of start.r:60-66, LambdaDisp from its values up to 4: the bound below covers the summation and the
    logarithms, and with a dispersion of 50 or more the lgamma terms of dnbinom (about 2000, one ulp 2e-13) cancel to
    leave two correct implementations a relative 1e-13 apart in the overhang vector before any term is summed
    (test_loglik_at_the_large_dispersions_against_the_exact_value covers those)."""
    x = rng.uniform(size=(n, 7))
    x[:, M.DISP] = rng.choice(M.DISP_STARTS[:5], n)
    x[:, M.RHO] = rng.choice(M.RHO_STARTS, n)
    return x


def loglik_cells():
    """The cells of 24 rows and a fixed nick vector keep the names (and the 200 vectors) they have always had."""
    cells = []
    for m in (24, 65, 66, 130, 256):
        for nu_kind in ("fixed", "raw"):
            for termini in ("both", "5p", "3p"):
                if termini == "both" and m % 2:
                    continue
                for jc in (False, True):
                    name = "%s-%s" % (termini, "jc" if jc else "hky")
                    if (m, nu_kind) != (24, "fixed"):
                        name += "-m%d-%s" % (m, nu_kind)
                    cells.append(pytest.param(termini, jc, m, nu_kind, id=name))
    return cells


@pytest.mark.parametrize("termini,jukes_cantor,m,nu_kind", loglik_cells())
def test_loglik_matches_the_restatement(termini, jukes_cantor, m, nu_kind):
    """|device - restatement| <= K(m) 2^-53 sum |term| on tables of 10, 10^6 and 3 bases a row.

    K(24) = 512, as ever.  Beyond 24 rows the bound grants every rounding on the way to the sum what it grants at 24 rows
    (stats_cases.loglik_k): the roundings are the lane's summation, ceil(m / 4) + 6 deep; the cumsum of seq_prob, one
    addition a row of its side (m / 2 with both termini, m with one); and 16 ulp for the library calls behind a term
    (three lgamma at 4, log, log1p, exp and the term's own log at 1).  So K(m) = ceil(512 ops(m) / ops(24)), with
    ops(m) = ceil(m / 4) + 6 + rows of a side + 16: both termini 922, 1536, 2740 at m = 66, 130, 256; one end 1024, 1034,
    1822, 3368 at m = 65, 66, 130, 256.  m = 65 .. 256 make the strided loops take a second to fourth trip, 65, 66 and 130
    leave the four row groups of the likelihood with different trip counts, and the raw nick vector keeps both halves
    of every pDam alive."""
    tables = loglik_tables(termini, m, nu_kind)
    nu = C.nu_of(nu_kind, m, termini, 40)
    opts = options(termini, m, jukes_cantor=jukes_cantor, diff_hangs=termini == "both", var_disp=True)
    mopts = M.Options(m, termini, jukes_cantor, termini == "both", True)
    n = 200 if (m, nu_kind) == (24, "fixed") else 50
    x = start_like_vectors(np.random.default_rng(17), n)
    params, table_of = np.repeat(x, 3, axis=0), np.tile(np.arange(3, dtype=np.int32), n)
    got = stats.loglik(tables, nu, C.ACGT, table_of, params, opts)
    consts = [M.lnfact_constant(t) for t in tables]
    k = C.loglik_k(m, termini)
    assert m != 24 or k == 512
    worst = 0.0
    for e in range(len(params)):
        want, total = M.loglik_of(tables[table_of[e]], consts[table_of[e]], nu, C.ACGT, mopts, params[e], with_abs=True)
        assert math.isfinite(want)
        bound = k * 2.0 ** -53 * total
        worst = max(worst, abs(got[e] - want) / bound)
        assert abs(got[e] - want) <= bound, (e, got[e], want, bound)
    print("worst |delta| / bound: %.3f" % worst)


BOUNDARY = {                                            # each value stands for one guard of the code
    "Lambda=0": {M.LAMBDA: 0.0},                        # dnbinom with prob 0: log(0), no mass anywhere
    "Lambda=1": {M.LAMBDA: 1.0},                        # dnbinom's prob == 1 early return
    "LambdaRight=0": {M.LAMBDAR: 0.0},
    "LambdaRight=1": {M.LAMBDAR: 1.0},
    "disp=0": {M.DISP: 0.0},                            # dnbinom's size == 0 early return
    "Theta=0": {M.THETA: 0.0},                          # the identity matrix: log(0) in every substitution
    "DeltaD=DeltaS=0": {M.DELTAD: 0.0, M.DELTAS: 0.0},  # pct = pga = 0
    "DeltaD=1": {M.DELTAD: 1.0},                        # the ranges' closed upper ends
    "DeltaS=1": {M.DELTAS: 1.0},
    "DeltaD=1,Lambda=1": {M.DELTAD: 1.0, M.LAMBDA: 1.0, M.LAMBDAR: 1.0},    # pct = 1 where nu = 1: log(0) in C.C
}


def value_class(v):
    return "nan" if math.isnan(v) else ("finite" if math.isfinite(v) else ("-inf" if v < 0 else "+inf"))


@pytest.mark.parametrize("jukes_cantor", [False, True], ids=["hky", "jc"])
@pytest.mark.parametrize("nu_kind", ["fixed", "raw"])
def test_loglik_boundary_values_have_the_restatements_class(nu_kind, jukes_cantor):
    """At the ends of the parameters' ranges the device and the restatement are both finite (and then within the bound of
    test_loglik_matches_the_restatement), both -inf or both NaN (0 log 0 on the table with empty cells, as in R)."""
    tables = loglik_tables("both", M24, nu_kind)
    nu = C.nu_of(nu_kind, M24, "both", 40)
    opts = options("both", jukes_cantor=jukes_cantor, diff_hangs=True, var_disp=True)
    mopts = M.Options(M24, "both", jukes_cantor, True, True)
    vectors = []
    for changes in BOUNDARY.values():
        v = np.array(C.TRUTH)
        for index, value in changes.items():
            v[index] = value
        vectors.append(v)
    params, table_of = np.repeat(np.stack(vectors), 3, axis=0), np.tile(np.arange(3, dtype=np.int32), len(vectors))
    got = stats.loglik(tables, nu, C.ACGT, table_of, params, opts)
    consts = [M.lnfact_constant(t) for t in tables]
    classes, worst = set(), 0.0
    for e, name in enumerate(np.repeat(list(BOUNDARY), 3)):
        want, total = M.loglik_of(tables[table_of[e]], consts[table_of[e]], nu, C.ACGT, mopts, params[e], with_abs=True)
        print("%-18s table %d: device %r restatement %r" % (name, table_of[e], got[e], want))
        assert value_class(got[e]) == value_class(want), (name, table_of[e], got[e], want)
        classes.add(value_class(want))
        if math.isfinite(want):
            bound = 512 * 2.0 ** -53 * total
            worst = max(worst, abs(got[e] - want) / bound)
            assert abs(got[e] - want) <= bound, (name, table_of[e], got[e], want, bound)
    assert classes == {"finite", "-inf", "nan"}, classes                  # (the cases reach every class)
    print("worst |delta| / bound: %.3f" % worst)


def test_loglik_at_the_large_dispersions_against_the_exact_value():
    """tests/golden/stats_loglik_exact.npz: 120 evaluations at the dispersions 50 .. 400 of the start search with their exact
    values (mpmath, tools/make_stats_exact.py).  The device stays within stats_cases.exact_bound of them, as the
    restatement does in tests/test_stats_host.py."""
    z = C.exact_fixture()
    worst = 0.0
    for g, m in enumerate(z["group_m"]):
        rows = np.flatnonzero(z["group_of"] == g)
        opts = options("both", int(m), diff_hangs=True, var_disp=True)
        got = stats.loglik(z["table_%d" % g][None], z["nu_%d" % g], z["acgt"], np.zeros(len(rows), np.int32), z["params"][rows], opts)
        for e, value in zip(rows, got):
            bound = C.exact_bound(int(m), "both", z["sum_abs"][e], z["sens"][e])
            ratio = abs(value - z["exact"][e]) / bound
            print("m %3d %-5s disp %3d: |device - exact| / bound %.4f" % (m, z["group_nu"][g], z["params"][e, M.DISP], ratio))
            worst = max(worst, ratio)
    print("worst |device - exact| / bound: %.4f" % worst)
    assert worst <= 1.0


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
    m, termini, flags, seed = C.PARITY[name][:4]
    r = C.parity_run(name)
    return stats.StatsOptions(seq_length=m // 2 if termini == "both" else m, termini=termini, rand=r["n_rand"], burn=r["n_burn"],
                              adjust=r["n_adjust"], iterations=r["n_iter"], fix_nicks=True, seed=seed, n_pred=2000, **flags, **kw)


@functools.lru_cache(maxsize=None)
def parity_device(name):
    table, nu, _, _, chain_id = C.parity_inputs(name)
    return stats.run_chains(table[None], nu, C.ACGT, parity_options(name), [chain_id])[0]


@pytest.mark.parametrize("name", list(C.PARITY))
def test_chain_follows_the_restatement(name):
    chain, want = C.parity_restatement(name)
    assert chain.margin > 1e-6, chain.margin            # no accept decision of the run is within rounding of its threshold
    got = parity_device(name)
    np.testing.assert_allclose(got.start[:7], chain.start, rtol=1e-12)
    np.testing.assert_allclose(got.trace, want, rtol=1e-9)
    np.testing.assert_allclose(got.prop_sd, chain.sd, rtol=0, atol=0)
    np.testing.assert_allclose(got.acc, [M.acc_rat(want[:, q]) for q in range(8)], rtol=1e-15)
    if name == "plain24":                               # no start search, no adjustment: the published values, untouched
        assert tuple(got.prop_sd) == M.PROPOSAL_SD
        assert tuple(got.start[:7]) == M.START


@pytest.mark.parametrize("name", [name for name in C.PARITY if name != "m2"])
def test_correcting_probabilities(name):
    """From the device's own trace and the same draws."""
    table, nu, mopts, seed, chain_id = C.parity_inputs(name)
    got = parity_device(name)
    rounds = max(C.parity_run(name)["n_adjust"], 1)
    want = M.correcting(got.trace, nu, C.ACGT, mopts, seed, chain_id, 2 + rounds, 2000)
    np.testing.assert_allclose(got.corr, want, rtol=1e-9)
    assert (got.corr >= 0).all() and (got.corr <= 1).all()
    if name in C.BEYOND_THE_WAVE:
        # the rows a lane keeps in its second to fourth sum: a device that never wrote them left zeros, and the columns
        # that are zero by the model (no C.T where nu = 0) would let zeros pass the comparison above
        assert got.corr.shape == (mopts.m, 2)
        for n in range(1, -(-mopts.m // 64)):
            rows = slice(64 * n, min(64 * n + 64, mopts.m))
            assert (want[rows].max(axis=1) > 0).all() and (got.corr[rows].max(axis=1) > 0).all(), n    # no row left at zero


# ---------------------------------------------------------------------- isolation and determinism
FIELDS = ("trace", "prop_sd", "acc", "corr", "start")


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
        for field in FIELDS:
            assert getattr(alone, field).tobytes() == getattr(other, field).tobytes(), field
    assert len(np.unique(alone.trace[:, M.DELTAS])) > 5
    other_seed = stats.StatsOptions(rand=3, burn=40, adjust=2, iterations=80, fix_nicks=True, diff_hangs=True, var_disp=True, seed=6, n_pred=100)
    assert run([6], other_seed).trace.tobytes() != alone.trace.tobytes()
    # (and the chain id is part of the key)
    assert stats.run_chains(tables[[6]], nu, C.ACGT, opts, [7])[0].trace.tobytes() != alone.trace.tobytes()


def test_a_chain_of_uneven_lane_trips_does_not_depend_on_its_launch():
    """m = 130: 65 rows a side (the strided loops' second trip holds one lane) and row groups of 33, 33, 32 and 32 trips in the
    likelihood, under a raw nick vector: the summation order is the chain's own here too."""
    m = 130
    opts = stats.StatsOptions(seq_length=m // 2, rand=3, burn=40, adjust=2, iterations=80, use_raw_nick_freq=True, diff_hangs=True,
                              var_disp=True, seed=5, n_pred=100)
    nus = np.stack([C.nu_of("raw", m, "both", 400 + k) for k in range(9)])
    tables = np.stack([C.model_table(m, "both", 500 + 10 * k, 400 + k, nu_kind="raw") for k in range(9)])
    ids = np.arange(9, dtype=np.uint32) + 100
    alone = stats.run_chains(tables[[4]], nus[[4]], C.ACGT, opts, ids[[4]])[0]
    among = stats.run_chains(tables, nus, C.ACGT, opts, ids)[4]
    for field in FIELDS:
        assert getattr(alone, field).tobytes() == getattr(among, field).tobytes(), field
    assert len(np.unique(alone.trace[:, M.LAMBDA])) > 5 and alone.corr[64:].any()       # (the chain moves its overhangs)


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


def test_stats_past_the_wave_from_the_command_line(cli_files, tmp_path):
    """--seq-length 35 with both termini: 70 rows, the nick vector of --use-raw-nick-freq.  The three files are what
    write_estimate makes of run_chains on the run's own tables."""
    from mapdamage_amd.main import main
    d, out, want = cli_files, tmp_path / "out", tmp_path / "want"
    flags = ["--use-raw-nick-freq"] + FAST[1:]
    assert main(["-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(out), "--stats", "--seq-length", "35", "--length", "70"]
                + flags) == 0
    positions, table = stats.data_matrix((out / "misincorporation.txt").read_text(), 35)
    assert positions == list(range(1, 36)) + list(range(-35, 0)) and table.shape == (70, 16)
    nu, warning = stats.nu_vector(table, use_raw_nick_freq=True)
    assert warning is None and 0 < nu.min() and nu.max() < 1              # the raw frequencies, not the constant fall-back
    opts = stats.StatsOptions(seq_length=35, rand=4, adjust=2, burn=100, iterations=200, use_raw_nick_freq=True, seed=9)
    estimate = stats.run_chains(table[None], nu, stats.read_base_freqs(out / "dnacomp_genome.csv"), opts, [0])[0]
    want.mkdir()
    stats.write_estimate(want, estimate, positions, opts)
    for name in CSVS:
        assert (out / name).read_bytes() == (want / name).read_bytes(), name
    assert len((out / stats.CORR_CSV).read_text().splitlines()) == 71      # the header and 70 rows
    assert estimate.corr[64:].any()
