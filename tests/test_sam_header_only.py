"""BAMReader(sam_header_only=True) — the header of SAM text for the device path, read without parsing the records: the same
libraries and references as the one-piece reader, and, when the host has to count after all, the same records."""
import os
import threading

import numpy as np

from mapdamage_amd import sam, synth
from mapdamage_amd.reader import BAMReader

RGS = [{"ID": "rgA", "SM": "s1", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s2", "LB": "lib2"}, {"ID": "x", "SM": "s1", "LB": "lib1"}]


def _files(tmp_path):
    ref, batch = synth.config1_batch()
    rg = [RGS[i % 3]["ID"] for i in range(batch.n)]
    path = tmp_path / "x.sam"
    sam.write_sam(str(path), batch, ref.names, ref.lengths, RGS, rg)
    return path


def test_header_only_reader_equals_the_one_piece_reader(tmp_path):
    path = _files(tmp_path)
    whole, head = BAMReader(path), BAMReader(path, sam_header_only=True)
    assert head.get_libraries() == whole.get_libraries()
    assert head.get_references() == whole.get_references()
    assert head.handle.batch.n == 0
    (a,), (b,) = list(whole.iter_batches()), list(head.iter_batches())
    for k in ("flag", "lib", "tid", "pos", "tlen", "cigar_off", "cigar", "seq_off", "seq", "qual"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    # (BAM and a fixed-size sample keep their own readers)
    assert BAMReader(path, sam_header_only=True, downsample_to=10).handle.batch.n > 0


def test_header_only_reader_on_a_pipe_keeps_the_stream(tmp_path):
    """On a stream the header is peeked: the records parsed behind it (from the first one, or from a line's offset) are the
    file's."""
    path = _files(tmp_path)
    data = path.read_bytes()
    whole = BAMReader(path)
    (want,) = list(whole.iter_batches())
    r, w = os.pipe()
    t = threading.Thread(target=lambda: (os.write(w, data), os.close(w)), daemon=True)
    t.start()
    try:
        reader = BAMReader("/dev/fd/%d" % r, sam_header_only=True)
        assert reader.get_libraries() == whole.get_libraries() and reader.get_references() == whole.get_references()
        assert reader._sam_body == data.index(b"\nr0\t") + 1
        (got,) = list(reader.iter_batches())
        reader.close()
    finally:
        t.join(timeout=60)
        os.close(r)
    for k in ("flag", "lib", "tid", "pos", "cigar", "seq"):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
