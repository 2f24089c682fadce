"""BAM from stdin and pipes on the device decode path (include/mdx.h mdx_source_*, mdx_gbam_open_source): the command line
reads `-i -`, a named pipe or /dev/fd/N once, decodes it on the GPU slab by slab, and writes the reference's tables; a host
decoder that takes over goes on where the device path stopped; damage ends in the file's error, never in a hang."""
import os
import pathlib
import subprocess
import sys
import threading

import numpy as np
import pytest

from mapdamage_amd import fasta, sam
from tests.test_pipe_input import _child, _feed, _write

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
FILES = ("misincorporation.txt", "dnacomp.txt", "lgdistribution.txt")
GOLDENS = [("config1_L70_A10_Q0", []), ("config1_merged_L70_A10_Q0", ["--merge-libraries"]), ("config1_L70_A10_Q20", ["-Q", "20"]),
           ("indelshapes_L70_A10_Q20", ["-Q", "20"]), ("indelshapes_L70_A10_Q0", []), ("edge_L70_A10_Q0", []), ("config4s_L70_A10", [])]


def _golden_bam(tmp_path, golden, extra):
    """The BAM and FASTA of a golden case, built as test_cli_gpu_decode_writes_the_reference_tables builds them."""
    from tests.util import Golden
    g = Golden(golden)
    rgs = [{"ID": "rg%d" % i, "SM": s, "LB": l} for i, (s, l) in enumerate(g.meta["libraries"])]
    raw_lib = np.load(str(ROOT / "tests" / "golden" / (golden + ".npz")))["lib"]
    if "--merge-libraries" in extra:
        rgs = [{"ID": "rg0", "SM": "a", "LB": "b"}, {"ID": "rg1", "SM": "c", "LB": "d"}]
        rg_of = ["rg%d" % (i % 2) for i in range(g.batch.n)]
    else:
        rg_of = ["rg%d" % int(l) for l in raw_lib]
    path = tmp_path / "in.bam"
    sam.write_bam(path, g.batch, g.ref.names, g.ref.lengths, rgs, rg_of)
    fasta.write_fasta(tmp_path / "ref.fa", g.ref)
    return g, path


def _cli(args, data=None, stdin_file=None, env=None, timeout=600):
    cmd = [sys.executable, "-m", "mapdamage_amd"] + [str(a) for a in args]
    e = dict(os.environ, **(env or {}))
    e["PYTHONPATH"] = str(ROOT) + os.pathsep + e.get("PYTHONPATH", "")
    if stdin_file is not None:
        with open(stdin_file, "rb") as fh:
            p = subprocess.run(cmd, stdin=fh, capture_output=True, timeout=timeout, env=e, cwd=str(ROOT))
        return p.stdout, p.stderr, p.returncode
    return _child(cmd, data, timeout, env=e, cwd=str(ROOT))


def _tables(out):
    return [(out / f).read_text() for f in FILES]


@pytest.mark.parametrize("golden,extra", GOLDENS)
def test_bam_on_stdin_gives_the_reference_tables(tmp_path, golden, extra):
    """`python -m mapdamage_amd -i -` with BAM written to its stdin through a pipe: the reference's three tables, byte for
    byte, decoded on the device."""
    g, path = _golden_bam(tmp_path, golden, extra)
    out = tmp_path / "out"
    _, err, rc = _cli(["-i", "-", "-r", tmp_path / "ref.fa", "-d", out, "--no-stats", "--log-level", "DEBUG"] + extra,
                      data=path.read_bytes())
    assert rc == 0, err.decode()
    for name in FILES:
        assert (out / name).read_text() == g.txt[name], name
    log = (out / "Runtime_log.txt").read_text()
    assert "Decode path: device; fallbacks from the device path: 0" in log
    assert "BAM from a stream" in log


def test_stdin_redirected_from_the_file_is_mapped(tmp_path):
    g, path = _golden_bam(tmp_path, "config1_L70_A10_Q20", ["-Q", "20"])
    out = tmp_path / "out"
    _, err, rc = _cli(["-i", "-", "-r", tmp_path / "ref.fa", "-d", out, "--no-stats", "-Q", "20", "--log-level", "DEBUG"],
                      stdin_file=path)
    assert rc == 0, err.decode()
    assert _tables(out) == [g.txt[f] for f in FILES]
    log = (out / "Runtime_log.txt").read_text()
    assert "stdin redirected from a regular file (mapped)" in log
    assert "Decode path: device; fallbacks from the device path: 0" in log


def _main_on_pipe(tmp_path, data, args, kind, seed=1):
    """``main([...])`` in process with ``-i`` a named pipe or /dev/fd/N that a writer thread feeds."""
    from mapdamage_amd.main import main
    if kind == "fifo":
        path = str(tmp_path / ("fifo%d" % seed))
        os.mkfifo(path)
        t = threading.Thread(target=lambda: _feed(os.open(path, os.O_WRONLY), data, seed), daemon=True)
        r = None
    else:
        r, w = os.pipe()
        path = "/dev/fd/%d" % r
        t = threading.Thread(target=_feed, args=(w, data, seed), daemon=True)
    t.start()
    try:
        rc = main(["-i", path] + [str(a) for a in args])
    finally:
        if r is not None:
            os.close(r)
        t.join(timeout=120)
    assert not t.is_alive()
    return rc


@pytest.mark.parametrize("kind", ["fifo", "devfd"])
def test_named_pipes_give_the_file_tables(tmp_path, kind):
    g, path = _golden_bam(tmp_path, "indelshapes_L70_A10_Q20", ["-Q", "20"])
    out = tmp_path / "out"
    assert _main_on_pipe(tmp_path, path.read_bytes(), ["-r", tmp_path / "ref.fa", "-d", out, "--no-stats", "-Q", "20",
                                                       "--log-level", "DEBUG"], kind) == 0
    assert _tables(out) == [g.txt[f] for f in FILES]
    assert "Decode path: device; fallbacks from the device path: 0" in (out / "Runtime_log.txt").read_text()


@pytest.mark.parametrize("layout", ["cut", "tiny"])
def test_many_slabs_of_a_stream(tmp_path, layout, monkeypatch):
    """A stream that spans many slabs (MDX_GBAM_SLAB_BYTES): -Q 20, --downsample 0.3 and -n 1000 give the tables of the same
    options on the file."""
    from mapdamage_amd import synth
    from mapdamage_amd.main import main
    ref = synth.make_genome(seed=11, sizes=(("chr1", 300_000), ("chr2", 100_000), ("chrS", 500)), n_run=500, lower_run=3000)
    fasta.write_fasta(tmp_path / "ref.fa", ref)
    path = _write(tmp_path, n=4000 if layout == "tiny" else 30_000, layout=layout)
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    for k, opts in enumerate((["-Q", "20"], ["--downsample", "0.3", "--downsample-seed", "7"], ["-n", "1000", "--downsample-seed", "7"])):
        base = ["-r", tmp_path / "ref.fa", "--no-stats", "--log-level", "DEBUG"] + opts
        assert main(["-i", str(path), "-d", str(tmp_path / ("file%d" % k))] + [str(a) for a in base]) == 0
        out = tmp_path / ("pipe%d" % k)
        assert _main_on_pipe(tmp_path, path.read_bytes(), ["-d", out] + base, "devfd", seed=k) == 0
        assert _tables(out) == _tables(tmp_path / ("file%d" % k)), opts
        log = (out / "Runtime_log.txt").read_text()
        if opts[0] != "-n":
            assert "Decode path: device; fallbacks from the device path: 0" in log, opts
        else:
            assert "Decode path: host decoder" in log


@pytest.mark.parametrize("extra", [[], ["--downsample", "0.3", "--downsample-seed", "7"]])
def test_the_fallback_on_a_stream_goes_on_where_the_device_stopped(tmp_path, extra, monkeypatch):
    """A slab the device path gives up on (MDX_GBAM_FAIL_AT): the host decoder takes the stream up at that slab's first
    record — the draws of --downsample with the run's one generator — and the tables are those of a run without it."""
    from mapdamage_amd import synth
    from mapdamage_amd.main import main
    ref = synth.make_genome(seed=11, sizes=(("chr1", 300_000), ("chr2", 100_000), ("chrS", 500)), n_run=500, lower_run=3000)
    fasta.write_fasta(tmp_path / "ref.fa", ref)
    path = _write(tmp_path, n=40_000, layout="cut")
    base = ["-r", tmp_path / "ref.fa", "--no-stats", "--log-level", "DEBUG", "--chunk-mb", "1"] + extra
    assert main(["-i", str(path), "-d", str(tmp_path / "file")] + [str(a) for a in base]) == 0
    for fail in ("0", "3"):
        monkeypatch.setenv("MDX_GBAM_FAIL_AT", fail)
        out = tmp_path / ("pipe" + fail)
        assert _main_on_pipe(tmp_path, path.read_bytes(), ["-d", out] + base, "devfd", seed=int(fail)) == 0
        assert _tables(out) == _tables(tmp_path / "file"), fail
        log = (out / "Runtime_log.txt").read_text()
        assert "WARNING GPU decode path gave up" in log and "from compressed offset" in log
        assert "the whole file again" not in log


def _last_line(err):
    lines = [x for x in err.decode(errors="replace").strip().splitlines() if x.strip()]
    return lines[-1] if lines else ""


def test_damaged_streams_end_in_the_files_error(tmp_path):
    """A truncated or damaged stream: the error text and exit status of the same bytes in a file, within the time limit."""
    from mapdamage_amd import synth
    ref = synth.make_genome(seed=11, sizes=(("chr1", 300_000), ("chr2", 100_000), ("chrS", 500)), n_run=500, lower_run=3000)
    fasta.write_fasta(tmp_path / "ref.fa", ref)
    raw = _write(tmp_path, n=30_000, layout="cut").read_bytes()
    bad = bytearray(raw)
    bad[len(raw) * 2 // 3] ^= 0x5A
    for name, data in (("truncated", raw[:len(raw) * 2 // 3 + 5]), ("damaged", bytes(bad))):
        f = tmp_path / (name + ".bam")
        f.write_bytes(data)
        args = ["-r", tmp_path / "ref.fa", "--no-stats", "--chunk-mb", "1"]
        _, err_f, rc_f = _cli(["-i", f, "-d", tmp_path / (name + "_f")] + args, data=b"")
        _, err_p, rc_p = _cli(["-i", "-", "-d", tmp_path / (name + "_p")] + args, data=data)
        assert rc_f != 0 and rc_p == rc_f, (name, err_p.decode()[-2000:])
        assert _last_line(err_p).replace("'-'", "X") == _last_line(err_f).replace(repr(str(f)), "X"), name


def test_refusals_on_a_pipe(tmp_path):
    g, path = _golden_bam(tmp_path, "config1_L70_A10_Q0", [])
    for extra, word in ((["--gpus", "2"], "--gpus 2"), (["--rescale-only"], "--rescale-only")):
        _, err, rc = _cli(["-i", "-", "-r", tmp_path / "ref.fa", "-d", tmp_path / "out", "--no-stats"] + extra,
                          data=path.read_bytes(), timeout=120)
        assert rc != 0
        assert word in err.decode() and "pipe" in err.decode()


def test_sam_on_stdin_still_gives_the_golden_tables(tmp_path):
    from tests.util import Golden
    g, _ = _golden_bam(tmp_path, "config1_L70_A10_Q20", ["-Q", "20"])
    rgs = [{"ID": "rg%d" % i, "SM": s, "LB": l} for i, (s, l) in enumerate(g.meta["libraries"])]
    raw_lib = np.load(str(ROOT / "tests" / "golden" / "config1_L70_A10_Q20.npz"))["lib"]
    samp = tmp_path / "in.sam"
    sam.write_sam(str(samp), g.batch, g.ref.names, g.ref.lengths, rgs, ["rg%d" % int(l) for l in raw_lib])
    out = tmp_path / "out"
    _, err, rc = _cli(["-i", "-", "-r", tmp_path / "ref.fa", "-d", out, "--no-stats", "-Q", "20"], data=samp.read_bytes())
    assert rc == 0, err.decode()
    assert _tables(out) == [Golden("config1_L70_A10_Q20").txt[f] for f in FILES]
