"""The host's share of the statistical stage (mapdamage_amd/stats.py) and its command-line gates: no GPU needed."""

import math
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import stats_model as M  # noqa: E402
from mapdamage_amd import stats  # noqa: E402
from util import Golden  # noqa: E402


# ---------------------------------------------------------------------- the data matrix
def hand_aggregation(text, seq_length, ends):
    """Column sums by (end, position), written apart from stats.data_matrix: a dictionary of integer lists."""
    lines = text.rstrip("\n").split("\n")
    names = lines[0].split("\t")
    sums = {}
    for line in lines[1:]:
        rec = dict(zip(names, line.split("\t")))
        if int(rec["Pos"]) > seq_length or rec["End"] not in ends:
            continue
        key = (rec["End"], int(rec["Pos"]))
        row = sums.setdefault(key, [0] * 16)
        for j, col in enumerate(stats.COLUMNS):
            row[j] += int(rec[col.replace(".", ">")])
    return sums


@pytest.mark.parametrize("termini,seq_length", [("both", 12), ("5p", 12), ("3p", 5), ("both", 1)])
def test_data_matrix_is_the_hand_aggregation(termini, seq_length):
    text = Golden("config1_L70_A10_Q0").txt["misincorporation.txt"]
    positions, table = stats.data_matrix(text, seq_length, termini)
    ends = ("5p", "3p") if termini == "both" else (termini,)
    want = hand_aggregation(text, seq_length, ends)
    expect = ([p for p in range(1, seq_length + 1)] if "5p" in ends else []) + \
             ([-p for p in range(seq_length, 0, -1)] if "3p" in ends else [])
    assert positions == expect
    assert table.shape == (len(expect), 16)
    for p, row in zip(positions, table):
        assert [int(v) for v in row] == want[("3p" if p < 0 else "5p", abs(p))]
    assert table.sum() > 0                                                  # (two libraries, two strands went into it)
    # the restatement's S matrices hold every base of a row once
    np.testing.assert_array_equal(M.counts(table).sum(axis=2), table[:, :4])


def test_lnfact_constant_agrees_with_the_restatement():
    _, table = stats.data_matrix(Golden("config1_L70_A10_Q0").txt["misincorporation.txt"], 12, "both")
    assert stats.lnfact_constant(table) == M.lnfact_constant(table)          # (both exactly rounded sums)


# ---------------------------------------------------------------------- the nick vector
def test_nu_vector_modes():
    table = np.ones((6, 16)) * 10
    table[:, :4] = 1000
    col = stats.COLUMNS.index
    table[:, col("C.T")] = [300, 200, 100, 10, 20, 30]
    table[:, col("G.A")] = [10, 20, 30, 100, 200, 300]
    assert stats.nu_vector(table, "both", single_stranded=True)[0].tolist() == [1] * 6
    assert stats.nu_vector(table, "both", fix_nicks=True)[0].tolist() == [1, 1, 1, 0, 0, 0]
    assert stats.nu_vector(table, "5p", fix_nicks=True)[0].tolist() == [1] * 6
    assert stats.nu_vector(table, "3p", fix_nicks=True)[0].tolist() == [0] * 6
    raw, warning = stats.nu_vector(table, "both", use_raw_nick_freq=True)
    assert warning is None
    np.testing.assert_allclose(raw, [300 / 310, 200 / 220, 100 / 130, 10 / 110, 20 / 220, 30 / 330], rtol=1e-15)
    with pytest.raises(stats.StatsError):
        stats.nu_vector(table, "both")                                      # the gam spline is not reproduced


def test_nu_vector_falls_back_when_a_ratio_is_nan():
    table = np.ones((4, 16)) * 10
    table[:, :4] = 1000
    table[2, stats.COLUMNS.index("C.T")] = table[2, stats.COLUMNS.index("G.A")] = 0          # 0 / 0 in row 2
    nu, warning = stats.nu_vector(table, "both", use_raw_nick_freq=True)
    assert nu.tolist() == [1, 1, 0, 0] and "constant nick frequency" in warning
    assert stats.nu_vector(table, "3p", use_raw_nick_freq=True)[0].tolist() == [0] * 4


# ---------------------------------------------------------------------- the files
def test_quantile7_is_numpys_default():
    rng = np.random.default_rng(3)
    probs = np.arange(41) * 0.025
    for n in (1, 2, 7, 1000):
        x = rng.normal(size=n)
        np.testing.assert_allclose(stats.quantile7(x, probs), np.quantile(x, probs), rtol=1e-14, atol=1e-15)


def test_written_files_round_trip(tmp_path):
    from mapdamage_amd.rescale import RescaleModel
    rng = np.random.default_rng(5)
    options = stats.StatsOptions(seq_length=3, fix_nicks=True, var_disp=True, iterations=40)
    trace = rng.uniform(size=(40, 8))
    trace[:, 7] = -1e5 - rng.uniform(size=40)
    corr = rng.uniform(size=(6, 2))
    positions = [1, 2, 3, -3, -2, -1]
    est = stats.Estimate(trace, np.ones(7), np.linspace(0.1, 0.8, 8), corr, trace[0])
    stats.write_estimate(tmp_path, est, positions, options)
    lines = (tmp_path / stats.CORR_CSV).read_text().splitlines()
    assert lines[0] == '"","Position","C.T","G.A"' and lines[1].startswith('"1",1,') and lines[6].startswith('"6",-1,')
    model = RescaleModel.from_csv(tmp_path / stats.CORR_CSV, 3, 3)
    for p, (c, g) in zip(positions, corr):
        assert model.corr_prob[("C", "T", p)] == pytest.approx(c, rel=1e-14)
        assert model.corr_prob[("G", "A", p)] == pytest.approx(g, rel=1e-14)
    # the trace: writeMCMC's columns in its order, rows named 1..n
    lines = (tmp_path / stats.ITER_CSV).read_text().splitlines()
    assert lines[0] == '"","Theta","DeltaD","DeltaS","Lambda","Rho","LambdaDisp","LogLik"'
    assert len(lines) == 41 and lines[40].startswith('"40",')
    back = np.array([[float(v) for v in line.split(",")[1:]] for line in lines[1:]])
    np.testing.assert_allclose(back, trace[:, [0, 2, 3, 4, 1, 6, 7]], rtol=1e-14)
    # the summary: mean, sd, acceptance ratio, 41 quantiles
    lines = (tmp_path / stats.SUMM_CSV).read_text().splitlines()
    names = [line.split(",")[0] for line in lines[1:]]
    assert names[:5] == ['"Mean"', '"Std."', '"Acceptance ratio"', '"0%"', '"2.5%"'] and names[-1] == '"100%"' and len(names) == 44
    summ = np.array([[float(v) for v in line.split(",")[1:]] for line in lines[1:]])
    orig = trace[:, [0, 2, 3, 4, 1, 6, 7]]
    np.testing.assert_allclose(summ[0], orig.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(summ[1], orig.std(axis=0, ddof=1), rtol=1e-13)
    np.testing.assert_allclose(summ[2], np.linspace(0.1, 0.8, 8)[[0, 2, 3, 4, 1, 6, 7]], rtol=1e-14)
    np.testing.assert_allclose(summ[3:], np.quantile(orig, np.arange(41) * 0.025, axis=0), rtol=1e-13)
    # --jukes-cantor, no --var-disp: four parameters and LogLik
    stats.write_estimate(tmp_path, est, positions, stats.StatsOptions(seq_length=3, fix_nicks=True, jukes_cantor=True, iterations=40))
    assert (tmp_path / stats.ITER_CSV).read_text().splitlines()[0] == '"","Theta","DeltaD","DeltaS","Lambda","LogLik"'


# ---------------------------------------------------------------------- the restatement's random numbers
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10."""
    assert [int(w) for w in M.philox(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(w) for w in M.philox(0xffffffff, 0xffffffff, *[0xffffffff] * 4)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(w) for w in M.philox(0xa4093822, 0x299f31d0, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    u0, u1 = M.uniforms(1, 2, 3, np.arange(1000), 5, 6)
    assert 0 < u0.min() and u0.max() < 1 and abs(u0.mean() - 0.5) < 0.05 and abs(np.corrcoef(u0, u1)[0, 1]) < 0.1


# ---------------------------------------------------------------------- the command line's gates
def parse(tmp_path, *args):
    from mapdamage_amd.main import parse_args
    return parse_args(["-i", str(tmp_path / "x.bam"), "-r", str(tmp_path / "ref.fa"), "-d", str(tmp_path / "out")] + list(args))


def test_stats_flags_are_accepted(tmp_path):
    """(The parent commit refused --rescale and --stats-only and did not know --stats.)"""
    o = parse(tmp_path, "--stats", "--fix-nicks", "--stats-seed", "7", "--rand", "3")
    assert o.want_stats and not o.no_stats and o.stats_options.seed == 7 and o.stats_options.rand == 3
    o = parse(tmp_path, "--rescale", "--single-stranded", "--reverse", "--seq-length", "9")
    assert not o.no_stats and o.termini == "3p" and o.stats_options.rows == 9
    assert o.rescale_out == tmp_path / "out" / "x.rescaled.bam" and o.rescale_length_5p == 9
    o = parse(tmp_path, "--stats", "--use-raw-nick-freq", "--diff-hangs", "--var-disp", "--jukes-cantor")
    c = o.stats_options.config(24)
    assert (c.m, c.termini, c.fix_ti_tv, c.same_overhangs, c.fix_disp, c.n_rand, c.n_adjust, c.n_burn, c.n_iter, c.n_pred) == \
        (24, 0, 1, 0, 0, 30, 10, 10000, 50000, 10000)
    # without the new flags nothing is estimated, as before
    assert parse(tmp_path).no_stats and parse(tmp_path, "--no-stats").no_stats


@pytest.mark.parametrize("args,message", [
    (["--stats"], "gam"),
    (["--rescale"], "--fix-nicks, --use-raw-nick-freq and --single-stranded"),
    (["--stats", "--fix-nicks", "--single-stranded"], "mutually exclusive"),
    (["--stats", "--use-raw-nick-freq", "--fix-nicks"], "mutually exclusive"),
    (["--stats", "--fix-nicks", "--diff-hangs", "--termini", "5p"], "Cannot use different overhangs with only the 5p end"),
    (["--stats", "--fix-nicks", "--diff-hangs", "--reverse"], "Cannot use different overhangs with only the 3p end"),
    (["--stats", "--fix-nicks", "--seq-length", "80"], "--seq-length"),
    (["--stats", "--fix-nicks", "--burn", "0"], "--burn"),
    (["--stats", "--fix-nicks", "--no-stats"], "--no-stats"),
    (["--plot-only"], "plotting"),
    (["--check-R-packages"], "plotting"),
])
def test_argument_errors(tmp_path, capsys, args, message):
    with pytest.raises(SystemExit) as exit_info:
        parse(tmp_path, *args)
    assert exit_info.value.code == 2
    assert message in capsys.readouterr().err


def test_stats_only_needs_a_folder(tmp_path, capsys):
    from mapdamage_amd.main import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--stats-only", "--fix-nicks"])
    assert "--folder required when using --stats-only" in capsys.readouterr().err
    (tmp_path / "dnacomp_genome.csv").write_text("A,C,G,T\r\n0.3,0.2,0.2,0.3\r\n")
    o = parse_args(["--stats-only", "--fix-nicks", "-d", str(tmp_path)])
    assert o.stats_only and not o.no_stats
    assert stats.read_base_freqs(tmp_path / "dnacomp_genome.csv") == [0.3, 0.2, 0.2, 0.3]


# ---------------------------------------------------------------------- the seeds of the GPU parity tests
def _parity_names():
    import stats_cases
    return list(stats_cases.PARITY)


@pytest.mark.parametrize("name", _parity_names())
def test_parity_cases_are_far_from_a_flipped_decision(name):
    """tests/test_gpu_stats.py compares device chains with the restatement at rtol 1e-9; the two can part only where an
    accept decision flips, so the cases are chosen with every decision at least 1e-6 away from its threshold."""
    import stats_cases
    chain, trace = stats_cases.parity_restatement(name)
    assert chain.margin > 1e-6, chain.margin
    assert np.isfinite(trace).all()
    # the chain moves: every free parameter is accepted now and then (in the first three cases; the later ones are there
    # for their row counts and models, and at least three of their parameters move)
    free = [p for p in range(7) if not ((p == M.RHO and chain.o.fix_ti_tv) or (p == M.LAMBDAR and chain.o.same_overhangs)
                                        or (p == M.DISP and chain.o.fix_disp))]
    if name in ("full", "m2", "5p"):
        for p in free:
            assert M.acc_rat(trace[:, p]) > 0.02, (p, M.acc_rat(trace[:, p]))
    else:
        assert sum(M.acc_rat(trace[:, p]) > 0.02 for p in free) >= 3
        assert all(np.all(trace[:, p] == trace[0, p]) for p in range(7) if p not in free)       # what the model fixes stays
        # the device's trace is held to rtol 1e-9 of this one; two LogLik values further apart than twice that cannot
        # coincide there, so the count of distinct values (the column's acceptance ratio, compared exactly) cannot differ
        assert stats_cases.loglik_gap(trace) > 2e-9, stats_cases.loglik_gap(trace)
    if name == "plain24":
        assert tuple(chain.start) == M.START and tuple(chain.sd) == M.PROPOSAL_SD


def test_parity_cases_cover_the_row_shapes():
    import stats_cases as C
    ms = {case[0] for case in C.PARITY.values()}
    assert max(ms) == stats.MAX_ROWS and {m % 4 for m in ms} == {0, 1, 2, 3} and C.BEYOND_THE_WAVE
    for kind, termini in (("raw", "both"), ("raw", "5p"), ("raw", "3p")):
        nu = C.nu_of(kind, 130, termini, 1)
        assert 0 < nu.min() and nu.max() < 1 and np.abs(nu - C.fixed_nu(130, termini)).max() <= 0.1
    assert C.nu_of("ones", 24, "both").tolist() == [1.0] * 24
    assert all(C.loglik_k(24, t) == 512 for t in ("both", "5p", "3p"))
    assert C.loglik_k(256, "both") == 2740 and C.loglik_k(256, "3p") == 3368 and C.loglik_k(65, "5p") == 1024


# ---------------------------------------------------------------------- the exact values of the large dispersions
def test_the_restatement_is_within_the_derived_bound_of_the_exact_values():
    """tests/golden/stats_loglik_exact.npz (tools/make_stats_exact.py): the numpy restatement against the mpmath values at the
    dispersions 50 .. 400, within stats_cases.exact_bound — the bound the device is held to in tests/test_gpu_stats.py."""
    import stats_cases as C
    z = C.exact_fixture()
    assert len(z["exact"]) == 120 and sorted(set(z["params"][:, M.DISP])) == [50, 100, 150, 400]
    worst = 0.0
    for g, m in enumerate(z["group_m"]):
        table, nu, mopts = z["table_%d" % g], z["nu_%d" % g], M.Options(int(m), "both", diff_hangs=True, var_disp=True)
        const = M.lnfact_constant(table)
        for e in np.flatnonzero(z["group_of"] == g):
            value, total = M.loglik_of(table, const, nu, z["acgt"], mopts, z["params"][e], with_abs=True)
            assert abs(total - z["sum_abs"][e]) <= 1e-9 * total
            ratio = abs(value - z["exact"][e]) / C.exact_bound(int(m), "both", z["sum_abs"][e], z["sens"][e])
            worst = max(worst, ratio)
            assert ratio <= 1.0, (e, value, z["exact_text"][e], ratio)
    print("worst |restatement - exact| / bound: %.4f" % worst)


def test_the_exact_values_are_reproduced_by_mpmath():
    pytest.importorskip("mpmath")
    import mpmath
    import stats_cases as C
    import stats_exact as X
    z = C.exact_fixture()
    for e in range(0, 120, 12):                         # ten of them: four at 24 rows, three at 130, three at 256
        g = int(z["group_of"][e])
        mopts = M.Options(int(z["group_m"][g]), "both", diff_hangs=True, var_disp=True)
        value, total, sens = X.loglik(z["table_%d" % g], z["nu_%d" % g], z["acgt"], mopts, z["params"][e])
        with mpmath.workdps(X.DIGITS):
            assert abs(value - mpmath.mpf(str(z["exact_text"][e]))) <= mpmath.mpf(10) ** -30
        assert float(value) == z["exact"][e] and float(total) == z["sum_abs"][e] and float(sens) == z["sens"][e]
