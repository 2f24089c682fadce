"""The device inflate and CRC32 stages alone (include/mdx.h mdx_gbam_inflate_blocks) on payloads a test supplies.  A
helper: it collects no tests (tests/test_gpu_decode.py, tests/test_gpu_inflate_craft.py)."""
import ctypes

import numpy as np


def inflate_blocks(eng, cases, out_offsets=None, out_bytes=None):
    """cases: [(deflate payload, ISIZE, CRC32)], their payloads packed back to back — what lies behind a block's input is the
    next block's.  out_offsets: where each block's output goes (default: one behind the other, each at a multiple of 16)
    in a buffer of out_bytes.  -> (status per block, the whole output buffer — the library fills it with 0xEE before the
    launch —, crc ok per block, the offsets)."""
    lib = eng._lib
    lib.mdx_gbam_inflate_blocks.restype = ctypes.c_int
    lib.mdx_gbam_inflate_blocks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    comp = np.frombuffer(b"".join(c for c, _, _ in cases) + b"\0" * 8, np.uint8).copy()
    blk = np.zeros((len(cases), 4), np.uint32)
    cin = cout = 0
    for i, (c, isize, _) in enumerate(cases):
        blk[i] = (cin, len(c), cout if out_offsets is None else out_offsets[i], isize)
        cin += len(c)
        cout += (isize + 15) & ~15
    if out_offsets is not None:
        cout = out_bytes
    out = np.zeros(cout + 16, np.uint8)
    status = np.zeros(len(cases), np.int32)
    crc = np.asarray([k for _, _, k in cases], np.uint32)
    crc_ok = np.zeros(len(cases), np.uint8)
    rc = lib.mdx_gbam_inflate_blocks(eng._ctx, comp.ctypes.data, cin, blk.ctypes.data, len(cases), out.ctypes.data, cout,
                                     status.ctypes.data, crc.ctypes.data, crc_ok.ctypes.data)
    assert rc == 0, rc
    return status, out[:cout], crc_ok.astype(bool), blk[:, 2].astype(np.int64)
