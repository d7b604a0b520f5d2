"""
What the guarded GPU modules (tests/test_gpu_guarded_*.py) share beside tests/_guarded.py: the stream and the synchronise
of a direct ctypes call, mxm_em_state arrays, the layout of a row-dictionary record (ONE place that knows it), and an
mxm_coded whose every device array is guarded.
"""
import numpy

from _guarded import guarded, guarded_2d, guarded_from

DEV = "cuda"
ENC_MAX_CODES = 256                         # table entries of a byte-coded record; beyond: 16-bit codes ("wide")


def load_lib():
    from mixemt_amd import _lib
    return _lib.load()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch
    torch.cuda.synchronize()


def check_all(bufs, what):
    """Guards of every buffer in the dict; a 2-D one also keeps its pad columns unchanged."""
    for name, buf in bufs.items():
        if hasattr(buf, "check_pads"):
            buf.check("%s %s" % (name, what), pads="unchanged")
        else:
            buf.check("%s %s" % (name, what))


def states(n, done=()):
    """mxm_em_state[n] (24 bytes each, 8-byte aligned), zeroed, with .done = 1 for the entries in `done` -> (buffer, raw)."""
    raw = numpy.zeros(n * 6, dtype=numpy.int32)
    for b in done:
        raw[6 * b] = 1
    return guarded_from(raw, numpy.int32, 8, DEV), raw


def read_states(buf, n):
    from mixemt_amd import _lib
    return list((_lib.EmState * n).from_buffer_copy(buf.get(numpy.uint8).tobytes()))


def is_sentinel(values):
    return bool((numpy.ascontiguousarray(values).view(numpy.uint8) == 0xFF).all())


def records(rec, rec_off, ndist, n_haps, limit, what):
    """The records of the rows with ndist > 0, each as (row, codes[H], P table[ndist], log table[ndist]):
        record = codes[ldc] (ldc = H rounded up to 8; 16-bit codes, 2 * ldc bytes, beyond 256 values) ++ P table ++ log table
    Asserts that every record lies inside [0, limit), 8-byte aligned, that no two overlap and that every code names a
    table entry.  -> (list of the tuples, sorted list of (begin, end) spans)."""
    ldc = (n_haps + 7) // 8 * 8
    out, spans = [], []
    for r in numpy.flatnonzero(ndist > 0):
        nd, off = int(ndist[r]), int(rec_off[r])
        code_bytes = ldc * (2 if nd > ENC_MAX_CODES else 1)
        size = code_bytes + 16 * nd
        assert 0 <= off and off + size <= limit and off % 8 == 0, (what, r, off, size, limit)
        spans.append((off, off + size))
        codes = rec[off:off + code_bytes].view(numpy.uint16 if nd > ENC_MAX_CODES else numpy.uint8)[:n_haps]
        assert int(codes.max()) < nd, (what, r)
        ptab = rec[off + code_bytes:off + code_bytes + 8 * nd].view(numpy.float64)
        mtab = rec[off + code_bytes + 8 * nd:off + size].view(numpy.float64)
        out.append((int(r), codes, ptab, mtab))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), what
    return out, spans


def encode_rows(lib, mat, ldm, rec_bytes, what):
    """mxm_encode_rows of a host matrix (M at a double's alignment, stride ldm) into guarded outputs -> (buffers, stats)."""
    n_rows, n_haps = mat.shape
    m_buf = guarded_2d(n_rows, n_haps, ldm, numpy.float64, 8, DEV).put(mat)
    out = {"rec": guarded(rec_bytes, 16, DEV), "rec_off": guarded(8 * n_rows, 8, DEV), "ndist": guarded(4 * n_rows, 4, DEV),
           "rowmax": guarded(8 * n_rows, 8, DEV), "stats": guarded(16, 8, DEV)}
    assert lib.mxm_encode_rows(m_buf.ptr, ldm, n_rows, n_haps, out["rec"].ptr, rec_bytes, out["rec_off"].ptr, out["ndist"].ptr,
                               out["rowmax"].ptr, out["stats"].ptr, stream()) == 0, lib.mxm_last_error()
    sync()
    m_buf.check("M " + what, pads="unchanged")
    check_all(out, what)
    return out, [int(v) for v in out["stats"].get(numpy.int64)]


def coded(lib, mat, wts, what):
    """Records in exactly mxm_coded_bytes, the dense rest linearised on the host, the wide-rows list: an mxm_coded whose
    every device array is guarded.  -> (struct, buffers to check, ndist, rest rows)."""
    from mixemt_amd import _lib
    n_rows, n_haps = mat.shape
    out, _ = encode_rows(lib, mat, n_haps + 3, lib.mxm_coded_bytes(n_rows, n_haps), what)
    ndist = out["ndist"].get(numpy.int32)
    rest = numpy.flatnonzero(ndist == 0)
    wide = numpy.flatnonzero(ndist > ENC_MAX_CODES).astype(numpy.int64)
    bufs = dict(out)
    ldp = n_haps + 2
    p_rest = w_rest = None
    if len(rest):
        top = mat[rest].max(axis=1)
        with numpy.errstate(under="ignore"):
            lin = numpy.exp(mat[rest] - numpy.where(numpy.isfinite(top), top, 0.0)[:, None])
        p_rest = bufs["P_rest"] = guarded_2d(len(rest), n_haps, ldp, numpy.float64, 16, DEV, pad=0).put(lin)
        w_rest = bufs["w_rest"] = guarded_from(wts[rest], numpy.float64, 8, DEV)
    if len(wide):
        bufs["wide_rows"] = guarded_from(wide, numpy.int64, 8, DEV)
    st = _lib.Coded(out["rec"].ptr, out["rec_off"].ptr, out["ndist"].ptr, n_rows, p_rest.ptr if len(rest) else None,
                    ldp if len(rest) else 0, w_rest.ptr if len(rest) else None, len(rest),
                    bufs["wide_rows"].ptr if len(wide) else None, len(wide))
    return st, bufs, ndist, rest
