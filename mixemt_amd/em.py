"""
EM mixture estimation on the GPU: the drop-in for `mixemt.em`
(reference: mixemt/em.py).  Same four entry points, same argument meaning:

    init_props(nhaps, alpha)                                   em.py:23
    converged(prop, last_prop, tolerance)                      em.py:39
    em_step(read_hap_mat, weights, ln_props, read_mix_mat)     em.py:57
    run_em(read_hap_mat, weights, args)                        em.py:94

Matrices may be numpy arrays (uploaded, results downloaded: drop-in behaviour)
or ROCm tensors (stay resident; `read_mix` comes back as a device tensor).

How the loop runs on the device (DESIGN.md has the derivation):
  * once per run_em:  P = exp(M - rowmax)            (mxm_linearize)
  * per iteration:    Z_r = sum_h p_h P_rh ; T_h = sum_r w_r P_rh / Z_r
                      (mxm_em_iter, one read of P, no transcendental)
                      ln p' = ln p + ln T - ln sum_h p T ; L1 test ; loop state on device,
                      kept as LOG proportions like the reference's (mxm_m_finalize)
  * after the loop:   posterior under theta_k in log space from M itself
                      (mxm_em_step), folded over runs with logaddexp.
All restarts of a multi-run advance in one device loop (mxm_em_loop); their
initial proportions are drawn on the host, sequentially, from numpy's global
legacy RNG exactly as the reference does (em.py:36, :123).
"""

import ctypes
import math
import os
import sys
import time

import numpy

from . import _lib
from ._dev import as_device, current_stream, device_empty, ptr, require_gpu, to_host, torch


def init_props(nhaps, alpha=1.0):
    """
    Random initial proportions (reference: em.py:23-36).  Stays on the host so
    the draw consumes numpy's process-global legacy stream like the reference
    (numpy.random.seed(args.seed) at bin/mixemt:507-508 must keep its meaning).
    """
    if alpha == float("inf"):
        return numpy.array([1.0 / nhaps] * nhaps)
    return numpy.random.dirichlet([alpha] * nhaps)


def converged(prop, last_prop, tolerance=0.0001):
    """
    sum_h |exp(prop_h) - exp(last_prop_h)| < tolerance on two LOG-proportion
    vectors (reference: em.py:39-54), evaluated by mxm_l1_exp_diff.
    """
    lib = _lib.load()
    dev = require_gpu()
    a = as_device(prop, torch.float64, dev)
    b = as_device(last_prop, torch.float64, dev)
    if a.numel() != b.numel():
        raise ValueError("operands could not be broadcast together")
    out = torch.empty(1, dtype=torch.float64, device=dev)
    _lib.check(lib.mxm_l1_exp_diff(a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(),
                                   current_stream()), "mxm_l1_exp_diff")
    return bool(out.item() < tolerance)


def _workspace(lib, n_rows, n_haps, n_runs, dev):
    nbytes = lib.mxm_workspace_bytes(n_rows, n_haps, n_runs)
    return torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev), nbytes


def em_step(read_hap_mat, weights, ln_props, read_mix_mat):
    """
    One EM step with the reference's semantics (em.py:57-91): fills
    `read_mix_mat` with the row-normalised log posterior and returns it with the
    new LOG proportions.  numpy in -> numpy out (read_mix_mat written in place);
    device tensors in -> device tensors out.
    """
    lib = _lib.load()
    dev = require_gpu()
    on_host = not isinstance(read_hap_mat, torch.Tensor)
    mat = as_device(read_hap_mat, torch.float64, dev)
    n_rows, n_haps = mat.shape
    wts = as_device(weights, torch.float64, dev)
    lnp = as_device(ln_props, torch.float64, dev)
    if wts.numel() != n_rows or lnp.numel() != n_haps:
        raise ValueError("em_step: weights/ln_props do not match the matrix shape")
    if on_host:
        out = torch.empty_like(mat)
    else:
        out = read_mix_mat
        if out.shape != mat.shape or out.dtype != torch.float64 or out.stride(1) != 1:
            raise ValueError("em_step: read_mix_mat must be a float64 matrix like read_hap_mat")
    colsum = torch.empty(n_haps, dtype=torch.float64, device=dev)
    ln_new = torch.empty(n_haps, dtype=torch.float64, device=dev)
    ws, ws_bytes = _workspace(lib, n_rows, n_haps, 1, dev)
    stream = current_stream()
    _lib.check(lib.mxm_em_step(mat.data_ptr(), mat.stride(0), wts.data_ptr(), lnp.data_ptr(),
                               n_rows, n_haps, out.data_ptr(), out.stride(0), 0,
                               colsum.data_ptr(), ws.data_ptr(), ws_bytes, stream),
               "mxm_em_step")
    _lib.check(lib.mxm_log_normalize(colsum.data_ptr(), n_haps, ln_new.data_ptr(), stream),
               "mxm_log_normalize")
    if on_host:
        read_mix_mat[...] = to_host(out)
        return read_mix_mat, ln_new.cpu().numpy()
    return out, ln_new


AUTO_CODED_MIN_CELLS = 1.5e7        # storage="auto": measured break-even of the one-launch loop over records against the
                                    # one-launch loops over the dense matrix (profiles/r04/small_runs_breakeven.txt: 26 vs 26 us
                                    # per iteration at 2400 x 5408, 31 vs 41 at 4600, 36 vs 58 at 7000; round 3, with the
                                    # records' iteration still four launches: 5e7)
# EmPlan.attach_quads: a quad dictionary beside the records ("auto" / True / False; the environment's MXM_QUADS = on / off / auto
# sets the start value: A/B runs of the tools without editing them)
QUADS = {"off": False, "0": False, "on": True, "1": True}.get(os.environ.get("MXM_QUADS", "auto").strip().lower(), "auto")
QUADS_MIN_ROWS = 300000             # ... "auto": from this many byte-coded rows (below, the one-launch loop over the records is faster)
QUADS_MIN_ROWS_MULTI = 20000        # ... with three or more restarts: tiles of three share a pass over the records (round 6), which beats the
                                    #     one-launch loop from the smallest record plans on (profiles/r06/multi_restart_routes.txt)
QUADS_MAX_FOOTPRINT = 60e9          # ... and only while records + dictionary stay under this many bytes
AUTO_CODED_MIN_CELLS_MULTI = 5e7    # ... with SEVERAL restarts: the one-launch records loop runs them one after
                                    # another while the dense path shares each pass of the matrix among up to four, so the
                                    # records only pay where an iteration is bound by the matrix's bytes (round 3's break-even)
AUTO_CODED_MAX_REST = 0.25          # ... and at most this share of the rows may stay dense


class EmPlan(object):
    """
    Device-resident inputs of the EM loop for one (rank-local) matrix:
    the log matrix, fp64 weights, the linearised copy and scratch.
    """

    def __init__(self, read_hap_mat, weights, n_runs=1, keep_log_matrix=True, storage="f64", records=None):
        """
        storage: element type of the linearised matrix the loop streams.
        "f64" (default) is the reference's arithmetic type end to end; "f32" is
        an opt-in variant that stores P as float (half the HBM traffic per
        iteration) and still multiplies and sums in fp64 -- measured within
        ~1e-8 of the fp64 path on the goldens, inside the 1e-6 parity bar, but
        NOT what the headline benchmark runs.  "coded" keeps every fp64 bit and
        stores each row as one byte per column plus the row's distinct values
        (mxm_encode_rows; 16-bit codes up to 1024 values, denser rows stay dense): the matrix
        build's rows hold a few dozen distinct sums, so the loop reads ~8x fewer
        bytes.  Matrices it does not apply to (fewer than 65 or more than 8192 columns)
        iterate as "f64".  "auto" = "coded" where it pays: more than 1.5 * 10^7 cells
        (below that the one-launch loops over the dense matrix are faster) and at
        most a quarter of the rows left dense by the encoder; otherwise "f64".
        `plan.storage` says what the plan iterates.
        records = preprocess.build_em_records_device(...)'s CodedMatrix: the matrix arrives in dictionary
        form straight from the build (no encode pass); read_hap_mat may then be None -- the posterior
        pass (em.posterior) then reads the records' log tables (mxm_em_step_coded).
        """
        if records is not None:
            self._from_records(records, read_hap_mat, weights, n_runs)
            return
        if storage not in ("f64", "f32", "coded", "auto"):
            raise ValueError("storage must be 'f64', 'f32', 'coded' or 'auto'")
        self.storage = storage
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.mat = as_device(read_hap_mat, torch.float64, self.dev)
        if self.mat.dim() != 2:
            raise ValueError("read_hap_mat must be 2-D")
        self.n_rows, self.n_haps = self.mat.shape
        self.wts = as_device(weights, torch.float64, self.dev)
        if self.wts.numel() != self.n_rows:
            raise ValueError("weights do not match the matrix height")
        self.n_runs = n_runs
        self.ws, self.ws_bytes = _workspace(self.lib, self.n_rows, self.n_haps, n_runs, self.dev)
        self.lin = None
        self.rowmax = None
        self.coded = None
        auto = storage == "auto"
        if auto:
            floor = AUTO_CODED_MIN_CELLS if n_runs <= 1 else AUTO_CODED_MIN_CELLS_MULTI
            storage = "coded" if (float(self.n_rows) * self.n_haps > floor) else "f64"
            self.storage = storage
        if storage == "coded":
            # (round 5: any width the linear kernels take, odd included, and any row stride -- an odd H, e.g. Build 17 plus
            # one custom haplogroup, used to fall back to the 7 x larger dense matrix here)
            if self.n_rows > 0 and self.lib.mxm_linear_supported(self.n_haps) and self.mat.stride(1) == 1:
                self.encode()
                if auto and self.coded_rest > AUTO_CODED_MAX_REST * self.n_rows:
                    self.coded = None                 # rows do not compress (not a build_em_matrix matrix): dense
                    self._coded_keep = self.coded_ndist = None
            if self.coded is None:
                self.storage = storage = "f64"
        if self.coded is not None:
            pass
        elif self.lib.mxm_linear_supported(self.n_haps) and self.n_rows > 0:
            self.rowmax = torch.empty(self.n_rows, dtype=torch.float64, device=self.dev)
            if storage == "f32":
                ldp = (self.n_haps + 3) // 4 * 4
                self.lin = device_empty((self.n_rows, ldp), torch.float32, self.dev, "the linearised matrix")
                _lib.check(self.lib.mxm_linearize_f32(self.mat.data_ptr(), self.mat.stride(0),
                                                      self.n_rows, self.n_haps, self.lin.data_ptr(),
                                                      self.lin.stride(0), self.rowmax.data_ptr(),
                                                      current_stream()), "mxm_linearize_f32")
            else:
                ldp = (self.n_haps + 1) // 2 * 2
                self.lin = device_empty((self.n_rows, ldp), torch.float64, self.dev, "the linearised matrix")
                _lib.check(self.lib.mxm_linearize(self.mat.data_ptr(), self.mat.stride(0),
                                                  self.n_rows, self.n_haps, self.lin.data_ptr(),
                                                  self.lin.stride(0), self.rowmax.data_ptr(),
                                                  current_stream()), "mxm_linearize")
        elif storage == "f32":
            self.storage = "f64"             # narrow matrices iterate the fp64 log-space kernel
        if not keep_log_matrix and (self.lin is not None or self.coded is not None):
            self.mat = None

    def _from_records(self, cm, read_hap_mat, weights, n_runs):
        """Plan over a matrix the build left as row-dictionary records (preprocess.CodedMatrix)."""
        self.storage = "coded"
        self.lib = _lib.load()
        self.dev = require_gpu()
        self.n_rows, self.n_haps = cm.n_rows, cm.n_haps
        self.mat = None if read_hap_mat is None else as_device(read_hap_mat, torch.float64, self.dev)
        if self.mat is not None and tuple(self.mat.shape) != (self.n_rows, self.n_haps):
            raise ValueError("read_hap_mat does not match the records")
        self.wts = as_device(weights, torch.float64, self.dev)
        if self.wts.numel() != self.n_rows:
            raise ValueError("weights do not match the matrix height")
        self.n_runs = n_runs
        self.ws, self.ws_bytes = _workspace(self.lib, self.n_rows, self.n_haps, n_runs, self.dev)
        self.lin = None
        self.rowmax = cm.rowmax
        n_rest = int(cm.rest_rows.numel())
        p_rest = w_rest = None
        if n_rest:
            ldp = (self.n_haps + 1) // 2 * 2
            p_rest = torch.empty((n_rest, ldp), dtype=torch.float64, device=self.dev)
            rm = torch.empty(n_rest, dtype=torch.float64, device=self.dev)
            _lib.check(self.lib.mxm_linearize(cm.m_rest.data_ptr(), cm.m_rest.stride(0), n_rest, self.n_haps,
                                              p_rest.data_ptr(), p_rest.stride(0), rm.data_ptr(), current_stream()),
                       "mxm_linearize")
            # the rest rows' weights: the library's own column gather over the weights as a 1 x R matrix (a torch
            # index_select here was the operator's first use in the process: ~5 ms of a paired-end plan's 14)
            if self.n_rows < 2 ** 31:
                cols = torch.from_numpy(cm.rest_rows.cpu().numpy().astype(numpy.int32)).to(self.dev)
                w_rest = torch.empty(n_rest, dtype=torch.float64, device=self.dev)
                _lib.check(self.lib.mxm_gather_columns(self.wts.data_ptr(), self.n_rows, 1, self.n_rows, cols.data_ptr(), n_rest,
                                                       w_rest.data_ptr(), n_rest, current_stream()), "mxm_gather_columns")
            else:
                w_rest = self.wts.index_select(0, cm.rest_rows).contiguous()
        self.coded_record_bytes = cm.used - 8 * int(cm.ndist_host().sum(dtype=numpy.int64))     # codes + P tables: the loop's read
        self.coded_bytes = self.coded_record_bytes + n_rest * self.n_haps * 8
        self.coded_rest = n_rest
        self.coded_ndist = cm.ndist
        wide = cm.wide_rows()
        self.coded_wide = int(wide.numel())
        self._coded_keep = (cm.rec, cm.rec_off, cm.ndist, p_rest, w_rest, cm, wide)
        self.records = cm
        self.coded = _lib.Coded(cm.rec.data_ptr(), cm.rec_off.data_ptr(), cm.ndist.data_ptr(), self.n_rows,
                                p_rest.data_ptr() if n_rest else None, p_rest.stride(0) if n_rest else 0,
                                w_rest.data_ptr() if n_rest else None, n_rest,
                                wide.data_ptr() if self.coded_wide else None, self.coded_wide)
        self._quad_keep = None
        self.attach_quads()

    def attach_quads(self, mode=None, cap=None, min_rows=None):
        """
        A quad dictionary beside the records, for the loop alone (include/mixemt_hip.h, mxm_build_quads;
        csrc/quad_kernels.hpp): one code byte per FOUR columns for the rows with at most 256 distinct value quadruples
        (98.8 % of build_em_matrix's byte-coded rows), 1.27 against 1.41 ms per pass at 10^6 x 5408.  The records stay
        complete -- every other consumer reads them -- so this costs memory: ~4.8 KB per row beside the records' 5.9.
        mode: True / False / "auto" (None = QUADS): auto builds them from QUADS_MIN_ROWS byte-coded rows while records +
        dictionary stay under QUADS_MAX_FOOTPRINT.  Measured at 10^6 x 5408 (profiles/r05/quads_product_1m.txt,
        pipeline_1m_records_quads.txt): the step 1.46 -> 1.32 ms, run_em's loop 1.44 (one-launch loop over the records) ->
        1.35 ms per iteration (the per-iteration kernels), the build 11 ms cold or warm in round 5 (encoder 8.6 ms; the row
        lists are formed on the device) and 4.3 ms since round 6 (a wave per row: 3.5 ms): a restart of ~400 iterations gains
        35 ms for it.
        cap: bytes of the first buffer (default: room for 112 quads per row; the kernel counts what it needs and an
        overflow repeats the build once with exactly that much).
        """
        mode = QUADS if mode is None else mode
        if self.coded is None or mode is False or self._quad_keep is not None:
            return self._quad_keep is not None
        lib, dev = self.lib, self.dev
        rec, rec_off, ndist = self._coded_keep[:3]
        nd_h = self.records.ndist_host() if getattr(self, "records", None) is not None else ndist.cpu().numpy()
        byte_coded = (nd_h > 0) & (nd_h <= 256)
        n_byte = int(byte_coded.sum())
        ldc = (self.n_haps + 7) // 8 * 8
        if n_byte == 0 or ldc // 4 > 6 * 256:         # (the quad pass is instantiated up to H = 6144)
            return False
        # room for >= 112 quads per row (mean on build_em_matrix rows: 93) + the 64 KB chunk every wave of the encoder (at most
        # 5120 of them) may leave half empty at the end
        # (a row's distinct quads go with its table entries: ~2 per entry on 150-bp reads -- 44 entries, 93 quads -- and on
        # merged pairs alike; a flat 112 made every paired-end build overflow and run twice)
        per_row = int(min(256, max(112, 2.3 * float(nd_h[byte_coded].mean()) + 12)))
        guess = n_byte * (2048 + 32 * per_row) + min(self.n_rows, 5120) * 65536 + (1 << 20)
        if mode == "auto":
            # by the card's TOTAL memory, not by what happens to be free: which loop runs decides the last bits of the sums
            # (fixed orders, but different ones), and the same call must take the same route every time
            # (min_rows: a caller whose loop runs the per-iteration kernels anyway -- dist.sharded_em_loop -- names its own
            # floor, and one restart is reason enough there)
            floor_ok = n_byte >= (min_rows if min_rows is not None else
                                  (QUADS_MIN_ROWS_MULTI if getattr(self, "n_runs", 1) >= 3 else QUADS_MIN_ROWS))
            # ... and not where it would take the process's device footprint past ~64 GB: the driver charges a process's
            # first growth past that mark with 2-6 s (profiles/r05/alloc_big.txt), more than the dictionary earns back
            if not floor_ok or int(rec.numel()) + guess > QUADS_MAX_FOOTPRINT:
                return False
        n_rows = self.n_rows
        laps = {} if os.environ.get("MXM_PIPELINE_TIMING") else None          # (synchronises: measurement only)
        self.quad_laps = laps
        t_lap = [time.perf_counter()]

        def lap(name):
            if laps is not None:
                torch.cuda.synchronize()
                laps[name] = round(laps.get(name, 0.0) + (time.perf_counter() - t_lap[0]) * 1e3, 2)
                t_lap[0] = time.perf_counter()

        qoff = torch.empty(n_rows, dtype=torch.int64, device=dev)
        nquad = torch.empty(n_rows, dtype=torch.int32, device=dev)
        stats = torch.empty(2, dtype=torch.int64, device=dev)
        cap = guess if cap is None else max(32, int(cap) // 32 * 32)
        for attempt in (0, 1):
            try:
                qrec = device_empty((cap,), torch.uint8, dev, "the quad dictionary")
            except ValueError:
                if mode == "auto":                    # no room beside the records: the records alone
                    return False
                raise
            lap("buffers")
            _lib.check(lib.mxm_build_quads(ctypes.byref(self.coded), self.n_haps, qrec.data_ptr(), qrec.numel(), qoff.data_ptr(),
                                           nquad.data_ptr(), stats.data_ptr(), current_stream()), "mxm_build_quads")
            used, n_left = (int(v) for v in stats.cpu())
            lap("quad_encode_kernel")
            if used <= cap:
                break
            if attempt == 1:
                raise ValueError("mxm_build_quads: buffer of %d bytes overflowed (%d needed)" % (cap, used))
            del qrec
            cap = (used + (256 << 20) + 31) // 32 * 32    # (the encoder reserves in chunks: a second run lays them out anew)
        # the row lists: formed on the device, ascending (mxm_quad_lists) -- their upload from the host was the build's
        # largest cold cost (a process's first copies from fresh pageable memory: 20-30 ms each, profiles/r05/quad_build_1m.txt)
        quad_rows_d = torch.empty(n_rows, dtype=torch.int64, device=dev)
        byte_rows_d = torch.empty(n_rows, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        sbytes = lib.mxm_quad_lists_scratch_bytes(n_rows)
        scratch = torch.empty(max(1, (sbytes + 7) // 8), dtype=torch.int64, device=dev)
        _lib.check(lib.mxm_quad_lists(ndist.data_ptr(), nquad.data_ptr(), n_rows, quad_rows_d.data_ptr(), byte_rows_d.data_ptr(),
                                      counts.data_ptr(), scratch.data_ptr(), scratch.numel() * 8, current_stream()), "mxm_quad_lists")
        n_quad, n_byte_left = (int(v) for v in counts.cpu())
        lap("row lists (device)")
        if n_quad == 0:
            return False
        #  run_em's loop only leaves the one-launch loop over the records for a dictionary of at least
        # mxm_quad_loop_min_rows() rows WITH quads -- "auto" decides by that same quantity, now that it is known, instead of
        # keeping a dictionary (4 ms, 4.8 KB per row) the loop would never look at; a caller that named its own floor
        # (dist.sharded_em_loop: its only loop is the per-iteration kernels) keeps what it asked for
        if mode == "auto" and min_rows is None and n_quad < int(lib.mxm_quad_loop_min_rows(int(getattr(self, "n_runs", 1)))):
            return False
        quad_rows_d, byte_rows_d = quad_rows_d[:n_quad], byte_rows_d[:n_byte_left]
        self._quad_keep = (qrec, qoff, nquad, quad_rows_d, byte_rows_d)
        self.coded.qrec, self.coded.qoff, self.coded.nquad = qrec.data_ptr(), qoff.data_ptr(), nquad.data_ptr()
        self.coded.quad_rows, self.coded.n_quad_rows = quad_rows_d.data_ptr(), n_quad
        self.coded.byte_rows, self.coded.n_byte_rows = (byte_rows_d.data_ptr() if n_byte_left else None), n_byte_left
        if laps is not None:
            laps["quads per row (room for / used, table entries)"] = "%d / %.1f, %.1f" % (
                per_row, (used / max(1, n_quad) - 2048) / 32.0, float(nd_h[byte_coded].mean()))
            sys.stderr.write("[attach_quads] %s\n" % laps)
        self.quad_rows_n = n_quad
        # what an iteration reads now -- the quad records, and of the records only the rows without quads (codes + P table):
        # reporting figures (bench.py, the tools), counted from nquad on the host when somebody asks; the plan itself does
        # not need them (1.3 ms of a 12 ms plan stage at 10^6 rows)
        rest_bytes = self.coded_rest * self.n_haps * 8

        def account():
            nq_h = nquad.cpu().numpy()
            left = byte_coded & (nq_h == 0)
            wide_h = nd_h > 256
            rec_left = int((ldc + 8 * nd_h[left].astype(numpy.int64)).sum() + (2 * ldc + 8 * nd_h[wide_h].astype(numpy.int64)).sum())
            quad_exact = int((2048 + 32 * nq_h[nq_h > 0].astype(numpy.int64)).sum())   # (`used` includes the allocator's slack)
            return {"quad_bytes": quad_exact, "coded_record_bytes": quad_exact + rec_left,
                    "coded_bytes": quad_exact + rec_left + rest_bytes}

        self._accounting = account
        for name in ("quad_bytes", "coded_record_bytes", "coded_bytes"):
            self.__dict__.pop(name, None)             # (the records' own figures: replaced by the ones counted on demand)
        return True

    def __getattr__(self, name):
        # quad_bytes / coded_record_bytes / coded_bytes after attach_quads: counted on first use (see there)
        if name in ("quad_bytes", "coded_record_bytes", "coded_bytes"):
            account = self.__dict__.get("_accounting")
            if account is not None:
                self.__dict__.update(account())
                self.__dict__["_accounting"] = None
                return self.__dict__[name]
        raise AttributeError(name)

    def encode(self):
        """Row-dictionary form of this plan's matrix (mxm_encode_rows) + the dense rest."""
        lib, dev, n_rows, n_haps = self.lib, self.dev, self.n_rows, self.n_haps
        # the record buffer: room for 64 table entries per row (mean on build_em_matrix rows: 27) instead of the worst
        # case (mxm_coded_bytes: 27 KB per row); the encoder counts what it would have needed, and an overflow
        # repeats the pass once with exactly that much
        ldc = (n_haps + 7) // 8 * 8
        one = 2 * ldc + 16 * 1024
        if self.coded is not None:                    # encoding again (bench.py times the second run): same buffers
            rec, rec_off, ndist = self._coded_keep[:3]
            cap = rec.numel()
        else:
            cap = max(one, min(lib.mxm_coded_bytes(n_rows, n_haps), n_rows * (ldc + 16 * 96) + (1 << 20)))
            rec = device_empty((cap,), torch.uint8, dev, "the coded matrix")
            rec_off = torch.empty(n_rows, dtype=torch.int64, device=dev)
            ndist = torch.empty(n_rows, dtype=torch.int32, device=dev)
            self.rowmax = torch.empty(n_rows, dtype=torch.float64, device=dev)
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        for attempt in (0, 1):
            _lib.check(lib.mxm_encode_rows(self.mat.data_ptr(), self.mat.stride(0), n_rows, n_haps, rec.data_ptr(), cap,
                                           rec_off.data_ptr(), ndist.data_ptr(), self.rowmax.data_ptr(), stats.data_ptr(),
                                           current_stream()), "mxm_encode_rows")
            used, n_rest = (int(v) for v in stats.cpu())
            if used <= cap:
                break
            if attempt == 1:
                raise ValueError("mxm_encode_rows: record buffer of %d bytes overflowed (%d needed)" % (cap, used))
            del rec
            cap = max(one, used)
            rec = device_empty((cap,), torch.uint8, dev, "the coded matrix")
        p_rest = w_rest = None
        if n_rest:
            # rows with more than 1024 distinct values: dense, in row order (fixed -> same sums on every run)
            idx = torch.nonzero(ndist == 0).flatten()
            m_rest = self.mat.index_select(0, idx)
            ldp = (n_haps + 1) // 2 * 2
            p_rest = torch.empty((n_rest, ldp), dtype=torch.float64, device=dev)
            rm = torch.empty(n_rest, dtype=torch.float64, device=dev)
            _lib.check(lib.mxm_linearize(m_rest.data_ptr(), m_rest.stride(0), n_rest, n_haps, p_rest.data_ptr(),
                                         p_rest.stride(0), rm.data_ptr(), current_stream()), "mxm_linearize")
            w_rest = self.wts.index_select(0, idx).contiguous()
        # what em_iter_coded_kernel reads per pass: codes + P tables (the records' log tables are for other passes)
        self.coded_record_bytes = used - 8 * int(ndist.sum().item())
        self.coded_bytes = self.coded_record_bytes + (n_rest * n_haps * 8)
        self.coded_rest = n_rest
        # rows with 16-bit codes (257..1024 values), in row order: the EM kernel takes them in a loop of their own
        wide = torch.nonzero(ndist > 256).flatten()
        self.coded_wide = int(wide.numel())
        self._coded_keep = (rec, rec_off, ndist, p_rest, w_rest, wide)      # the tensors self.coded points into
        self.coded_ndist = ndist                      # [R] int32: table entries per row, 0 = the row stays dense
        self.coded = _lib.Coded(rec.data_ptr(), rec_off.data_ptr(), ndist.data_ptr(), n_rows,
                                p_rest.data_ptr() if n_rest else None, p_rest.stride(0) if n_rest else 0,
                                w_rest.data_ptr() if n_rest else None, n_rest,
                                wide.data_ptr() if self.coded_wide else None, self.coded_wide)
        self._quad_keep = None                        # (a second encode(): the quads are made again from the new records)
        self.attach_quads()

    # pointers for the C ABI ------------------------------------------------
    def mat_args(self):
        if self.mat is None:
            return 0, 0
        return self.mat.data_ptr(), self.mat.stride(0)

    def lin_args(self):
        if self.lin is None:
            return 0, 0
        return self.lin.data_ptr(), self.lin.stride(0)

    def release_linear(self):
        """
        Hand the linearised matrix's storage over for reuse as an [R][H] fp64 buffer (the
        posterior matrix run_em returns has exactly that shape): the plan cannot iterate
        afterwards.  None if there is no such buffer (narrow matrix, fp32 storage, padded rows).
        A 43 GB hipMalloc costs ~1.2 s -- half the EM loop's time at 10^6 x 5408.
        """
        lin = self.lin
        if lin is None or lin.dtype != torch.float64 or lin.stride(0) != self.n_haps:
            return None
        self.lin = None
        self.spent = True
        return lin

    def restart_tile(self):
        """Restarts that share one pass over this plan's matrix (mxm_restart_tile / mxm_restart_tile_coded; 1 for the
        fp32-storage variant, for narrow matrices and for records without a quad dictionary, which iterate one restart per pass)."""
        if self.coded is not None:                    # records: three beside a quad dictionary (em_iter_quad_batched_kernel), else one
            return int(self.lib.mxm_restart_tile_coded(ctypes.byref(self.coded), self.n_haps))
        if self.lin is None or self.storage != "f64":
            return 1
        return int(self.lib.mxm_restart_tile(self.n_haps))

    # buffers (the surface dist.sharded_em_loop drives) ----------------------
    def alloc_props(self, host):
        return torch.from_numpy(numpy.ascontiguousarray(host, dtype=numpy.float64)).to(self.dev)

    def alloc_state(self, n_runs):
        return new_state(n_runs, self.dev)

    def read_state(self, state):
        return read_state(state)

    def em_iter(self, props, ln_props, state, colsum):
        """Enqueue one fused E+M step for every restart (mxm_em_iter): colsum <- the
        unscaled column sums T (see include/mixemt_hip.h)."""
        if getattr(self, "spent", False):
            raise ValueError("this plan's linearised matrix has been released (release_linear)")
        m_ptr, ldm = self.mat_args()
        p_ptr, ldp = self.lin_args()
        if self.coded is not None:
            _lib.check(self.lib.mxm_em_iter_coded(ctypes.byref(self.coded), self.wts.data_ptr(), props.data_ptr(),
                                                  self.n_haps, props.shape[0], ptr(state), colsum.data_ptr(),
                                                  self.ws.data_ptr(), self.ws_bytes, current_stream()),
                       "mxm_em_iter_coded")
            return
        if self.storage == "f32":
            _lib.check(self.lib.mxm_em_iter_f32(p_ptr, ldp, self.wts.data_ptr(), props.data_ptr(),
                                                self.n_rows, self.n_haps, props.shape[0], ptr(state),
                                                colsum.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                                current_stream()), "mxm_em_iter_f32")
            return
        _lib.check(self.lib.mxm_em_iter(m_ptr, ldm, p_ptr, ldp, self.wts.data_ptr(),
                                        props.data_ptr(), ln_props.data_ptr(), self.n_rows,
                                        self.n_haps, props.shape[0], ptr(state), colsum.data_ptr(),
                                        self.ws.data_ptr(), self.ws_bytes, current_stream()),
                   "mxm_em_iter")

    def finalize(self, colsum, ln_cur, ln_new, props_cur, state, tol, max_iter):
        """Enqueue the M-step normalisation + convergence test (mxm_m_finalize)."""
        _lib.check(self.lib.mxm_m_finalize(colsum.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(),
                                           props_cur.data_ptr(), self.n_haps, props_cur.shape[0],
                                           float(tol), int(max_iter), state.data_ptr(),
                                           current_stream()), "mxm_m_finalize")


def new_state(n_runs, dev):
    """Device array of mxm_em_state (24 bytes each), zeroed."""
    return torch.zeros(n_runs * (ctypes.sizeof(_lib.EmState) // 8), dtype=torch.int64, device=dev)


def read_state(state):
    """Device mxm_em_state array -> list of (done, iters, l1)."""
    raw = state.cpu().numpy().tobytes()
    n = len(raw) // ctypes.sizeof(_lib.EmState)
    arr = (_lib.EmState * n).from_buffer_copy(raw)
    if any(s.error == 2 for s in arr):
        raise ValueError("EM loop state: the one-shot exchange timed out waiting for a rank (mxm_exchange_pull poisoned the sums)")
    if any(s.error for s in arr):
        raise ValueError("EM loop state: the records' wide_rows list does not match the rows with more than 256 values "
                         "(mxm_em_iter_coded poisoned the sums)")
    return [(s.done, s.iters, s.l1) for s in arr]


def log_inits(inits):
    """Initial LOG proportions exactly as the reference forms them (numpy.log on the host,
    em.py:123-124) and the linear copy the streaming kernel multiplies with."""
    with numpy.errstate(divide="ignore"):
        ln0 = numpy.log(numpy.ascontiguousarray(inits, dtype=numpy.float64))
    return ln0, numpy.exp(ln0)


def em_loop(plan, inits, tolerance, max_iter, check_every=16):
    """
    The run_em inner loop (em.py:126-143) for all restarts at once on one GPU.
    inits: [B][H] linear initial proportions.  Returns
    (ln_cur = log theta_k, ln_new = log theta_{k+1}, [(done, iters, l1)] per run).
    """
    lib, dev = plan.lib, plan.dev
    if getattr(plan, "spent", False):
        raise ValueError("this plan's linearised matrix has been released (release_linear)")
    ln0, p0 = log_inits(inits)
    n_runs, n_haps = ln0.shape
    props_cur = torch.from_numpy(p0).to(dev)
    ln_cur = torch.from_numpy(ln0).to(dev)
    ln_new = ln_cur.clone()
    colsum = torch.zeros_like(props_cur)
    state = new_state(n_runs, dev)
    host_state = (_lib.EmState * n_runs)()
    if max_iter > 0 and plan.coded is not None:
        _lib.check(lib.mxm_em_loop_coded(ctypes.byref(plan.coded), plan.wts.data_ptr(), n_haps, n_runs,
                                         props_cur.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(),
                                         colsum.data_ptr(), state.data_ptr(), float(tolerance),
                                         int(max_iter), int(check_every), plan.ws.data_ptr(),
                                         plan.ws_bytes, current_stream(), host_state), "mxm_em_loop_coded")
    elif max_iter > 0 and plan.storage == "f32":
        p_ptr, ldp = plan.lin_args()
        _lib.check(lib.mxm_em_loop_f32(p_ptr, ldp, plan.wts.data_ptr(), plan.n_rows, n_haps, n_runs,
                                       props_cur.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(),
                                       colsum.data_ptr(), state.data_ptr(), float(tolerance),
                                       int(max_iter), int(check_every), plan.ws.data_ptr(),
                                       plan.ws_bytes, current_stream(), host_state), "mxm_em_loop_f32")
    elif max_iter > 0:
        m_ptr, ldm = plan.mat_args()
        p_ptr, ldp = plan.lin_args()
        _lib.check(lib.mxm_em_loop(m_ptr, ldm, p_ptr, ldp, plan.wts.data_ptr(), plan.n_rows,
                                   n_haps, n_runs, props_cur.data_ptr(), ln_cur.data_ptr(),
                                   ln_new.data_ptr(), colsum.data_ptr(), state.data_ptr(),
                                   float(tolerance), int(max_iter), int(check_every),
                                   plan.ws.data_ptr(), plan.ws_bytes, current_stream(), host_state),
                   "mxm_em_loop")
    states = [(s.done, s.iters, s.l1) for s in host_state]
    return ln_cur, ln_new, states


def posterior(plan, ln_theta, out=None, fold=False):
    """
    Log posterior under log-proportions `ln_theta` (em.py:80-83) written to
    `out` (mode store) or folded into it with logaddexp (em.py:156).
    """
    lnp = as_device(ln_theta, torch.float64, plan.dev)
    if out is None:
        out = device_empty((plan.n_rows, plan.n_haps), torch.float64, plan.dev, "the posterior matrix")
    if plan.mat is None and getattr(plan, "records", None) is not None:
        # the matrix exists only as records: coded rows from their log tables, the rest from their dense copies
        cm = plan.records
        lnp = lnp.reshape(-1).contiguous()
        coded = cm.struct()
        props_d = torch.exp(lnp)
        n_rest = int(cm.rest_rows.numel())
        _lib.check(plan.lib.mxm_em_step_coded(ctypes.byref(coded), plan.n_haps, lnp.data_ptr(), props_d.data_ptr(),
                                              cm.rowmax.data_ptr(), cm.m_rest.data_ptr() if n_rest else 0,
                                              cm.m_rest.stride(0) if n_rest else 0,
                                              cm.rest_rows.data_ptr() if n_rest else 0, n_rest,
                                              out.data_ptr(), out.stride(0), 1 if fold else 0,
                                              current_stream()), "mxm_em_step_coded")
        return out
    if plan.mat is None:
        raise ValueError("posterior pass needs the log matrix (keep_log_matrix=True)")
    _lib.check(plan.lib.mxm_em_step(plan.mat.data_ptr(), plan.mat.stride(0), 0, lnp.data_ptr(),
                                    plan.n_rows, plan.n_haps, out.data_ptr(), out.stride(0),
                                    1 if fold else 0, 0, 0, 0, current_stream()),
               "mxm_em_step")
    return out


class RecordsPosterior(object):
    """
    run_em's returned posterior (em.py:145-165: the E-step under every run's theta_k, folded with logaddexp, minus
    log n_multi) for a matrix that exists only as records, formed on demand for a range of rows -- what
    run_em_ex(..., records=cm, want_read_mix=False) did not materialise.  ln_theta_k: its "ln_theta_k" ([n_multi][H]).
    io.save_matrix / dump_all write it slab by slab (`-s` on the records route).
    """

    def __init__(self, cm, ln_theta_k):
        self.cm, self.rec = cm, cm.rec
        self.ln_theta_k = numpy.atleast_2d(numpy.asarray(ln_theta_k, dtype=numpy.float64))
        self.shape = (cm.n_rows, cm.n_haps)

    def dense(self, lo=0, hi=None):
        import types
        part = self.cm.rows(lo, self.cm.n_rows if hi is None else hi)
        lib = _lib.load()
        shim = types.SimpleNamespace(dev=self.rec.device, n_rows=part.n_rows, n_haps=self.cm.n_haps, mat=None,
                                     records=part, lib=lib)
        out = device_empty((part.n_rows, self.cm.n_haps), torch.float64, self.rec.device, "rows of the posterior matrix")
        if part.n_rows == 0:
            return out
        n_multi = self.ln_theta_k.shape[0]
        for run in range(n_multi):
            posterior(shim, self.ln_theta_k[run], out=out, fold=(run > 0))
        if n_multi > 1:
            _lib.check(lib.mxm_add_scalar(out.data_ptr(), out.stride(0), part.n_rows, self.cm.n_haps,
                                          -math.log(n_multi), current_stream()), "mxm_add_scalar")
        return out


def collect_result(plan, inits, ln_cur, ln_new, states, want_read_mix=True, verbose=False,
                   reuse_linear=False):
    """
    What run_em does after its loops (em.py:145-165): posterior under theta_k
    per run, folded with logaddexp, minus log n; proportions = exp(mean of the
    runs' LOG proportions) -- a geometric mean that is not renormalised.
    ln_cur / ln_new are the loop's log theta_k / log theta_{k+1}.
    reuse_linear: the loops are over, write the posterior into the linearised
    matrix's storage instead of a new allocation (the plan is spent afterwards).
    """
    n_multi, n_haps = inits.shape
    ln_k = ln_cur.cpu().numpy()
    ln_next = ln_new.cpu().numpy()
    if verbose:
        for run, (done, iters, _) in enumerate(states):
            sys.stderr.write("Starting EM run %d...\n" % (run + 1))
            sys.stderr.write("." * (iters // 10))
            if done == 1:
                sys.stderr.write("\nConverged! (%d)\n" % iters)
    read_mix = None
    if want_read_mix:
        if reuse_linear and plan.mat is not None:
            read_mix = plan.release_linear()          # overwritten by run 0's store below
        for run in range(n_multi):
            read_mix = posterior(plan, ln_k[run], out=read_mix, fold=(run > 0))
        if n_multi > 1:
            _lib.check(plan.lib.mxm_add_scalar(read_mix.data_ptr(), read_mix.stride(0),
                                               plan.n_rows, n_haps, -math.log(n_multi),
                                               current_stream()), "mxm_add_scalar")
    res = ln_next[0].copy()
    if n_multi > 1:
        for run in range(1, n_multi):
            res += ln_next[run]                       # em.py:155, in log space
        res /= n_multi
    props = numpy.exp(res)                            # em.py:163
    return {"props": props, "read_mix": read_mix, "iters": [s[1] for s in states],
            "done": [s[0] for s in states], "run_props": numpy.exp(ln_next), "inits": inits,
            "l1": [s[2] for s in states], "ln_theta_k": ln_k}


def run_em_ex(read_hap_mat, weights, args, inits=None, want_read_mix=True, storage=None, records=None):
    """
    run_em with the parity observables exposed.  Returns a dict:
        props      [H] numpy, linear (geometric mean over runs, em.py:155-163)
        read_mix   [R][H] device tensor, log (None if want_read_mix=False)
        iters      per-run iteration counts ("Converged! (n)", em.py:135)
        run_props  [n_multi][H] numpy, each run's theta_{k+1}
        inits      [n_multi][H] numpy, the initial draws
        done       per-run stop reason (1 converged, 2 max_iter)
        ln_theta_k [n_multi][H] numpy, log theta_k: the proportions the returned posterior is taken under (em.py:137-143)
    records: a preprocess.CodedMatrix (the build's row-dictionary output) to iterate instead of encoding
    read_hap_mat; read_hap_mat may then be None (the posterior comes from the records' log tables).
    storage: "f64" | "f32" | "coded" | "auto" (EmPlan); default args.storage, else "auto".
    """
    n_multi = int(args.n_multi)
    # "auto" (default since round 3, once golden g10 pinned that branch to a reference run): the dense fp64 matrix up to
    # 1.5e7 cells -- there the dense one-launch loops are the fastest form -- and lossless row dictionaries above, where an
    # iteration reads 8x fewer bytes (4.2x faster at 10^6 x 5408); same stopping iterations, proportions within 1e-9
    storage = storage or getattr(args, "storage", "auto")
    t_plan = time.perf_counter()
    plan = EmPlan(read_hap_mat, weights, n_runs=n_multi, storage=storage, records=records)
    torch.cuda.synchronize()
    t_plan = time.perf_counter() - t_plan
    if inits is None:
        # sequential draws in run order: same RNG consumption as em.py:123
        inits = numpy.stack([init_props(plan.n_haps, alpha=args.init_alpha)
                             for _ in range(n_multi)])
    inits = numpy.ascontiguousarray(inits, dtype=numpy.float64)
    verbose = getattr(args, "verbose", False)
    t_loop = time.perf_counter()
    if verbose:
        # The reference's own progress text (em.py:119-135): "Starting EM run i...", a dot per 10 iterations, "Converged! (n)",
        # run after run.  The restarts still advance TOGETHER in one batched loop -- the same kernels, summation orders and
        # bits as without -v (a logging flag must not change the arithmetic, nor cost n_multi times the passes
        # over the matrix) -- and the text follows the lowest run that is not fully reported yet: live for that run, caught
        # up at once for the runs that finished in its shadow.
        report = {"run": 0, "dots": 0, "open": False}

        def tell(iters_done, n_runs):
            """iters_done[i] = (iterations so far, done code) of run i"""
            while report["run"] < n_runs:
                run = report["run"]
                iters, done = iters_done[run]
                if not report["open"]:
                    sys.stderr.write("Starting EM run %d...\n" % (run + 1))
                    report["open"], report["dots"] = True, 0
                dots = iters // 10 - report["dots"]
                if dots > 0:
                    sys.stderr.write("." * dots)
                    report["dots"] += dots
                if done == 0:
                    break
                if done == 1:
                    sys.stderr.write("\nConverged! (%d)\n" % iters)
                report["run"], report["open"] = run + 1, False
            sys.stderr.flush()

        def on_state(state_host, n_runs, _user):
            tell([(state_host[i].iters, state_host[i].done) for i in range(n_runs)], n_runs)
        hook = _lib.PROGRESS_FN(on_state)
        try:
            plan.lib.mxm_set_progress_callback(ctypes.cast(hook, ctypes.c_void_p), None, 10)
            ln_cur, ln_new, states = em_loop(plan, inits, args.tolerance, args.max_iter)
        finally:
            plan.lib.mxm_set_progress_callback(None, None, 10)
        tell([(st[1], st[0]) for st in states], n_multi)               # whatever the last read-back did not show yet
    else:
        ln_cur, ln_new, states = em_loop(plan, inits, args.tolerance, args.max_iter)
    t_loop = time.perf_counter() - t_loop
    res = collect_result(plan, inits, ln_cur, ln_new, states, want_read_mix, False, reuse_linear=True)
    # where the call's time went: plan (allocations -- a 43 GB hipMalloc alone varies between 0.3 and 3 s
    # from process to process -- plus linearise / encode) and the loop itself (blocking, so wall time = device time)
    res["plan_s"], res["loop_s"], res["storage"] = t_plan, t_loop, plan.storage
    return res


class SampleBatch(object):
    """
    The rows of many samples back to back in ONE records matrix, for the batched loop (mxm_em_loop_samples):
        rec                        the record buffer every entry's offsets point into
        rec_off, ndist, wts [R]    the concatenated rows (an entry may REPEAT another's offsets: the restarts of one sample
                                   share its records, nothing is copied)
        row0 [S + 1] numpy int64   entry s owns the rows [row0[s], row0[s + 1])
    """

    def __init__(self, rec, rec_off, ndist, wts, row0, n_haps):
        self.lib = _lib.load()
        self.dev = rec.device
        self.rec, self.rec_off, self.ndist, self.wts = rec, rec_off.contiguous(), ndist.contiguous(), wts.contiguous()
        self.row0 = numpy.ascontiguousarray(row0, dtype=numpy.int64)
        self.n_entries, self.n_rows, self.n_haps = len(self.row0) - 1, int(self.row0[-1]), int(n_haps)
        if self.rec_off.numel() != self.n_rows or self.ndist.numel() != self.n_rows or self.wts.numel() != self.n_rows:
            raise ValueError("rec_off / ndist / weights do not match row0")
        nd_h = self.ndist.cpu().numpy()
        self.wide = torch.from_numpy(numpy.flatnonzero(nd_h > 256)).to(self.dev)
        n_wide = int(self.wide.numel())
        self.coded = _lib.Coded(self.rec.data_ptr(), self.rec_off.data_ptr(), self.ndist.data_ptr(), self.n_rows,
                                None, 0, None, 0, self.wide.data_ptr() if n_wide else None, n_wide)
        self.row0_ptr = self.row0.ctypes.data_as(ctypes.c_void_p)
        self.n_tiles = int(self.lib.mxm_samples_plan(self.row0_ptr, self.n_entries, None, 0, None))
        if self.n_tiles < 0:
            raise ValueError("mxm_samples_plan failed: %s" % self.lib.mxm_last_error().decode("utf-8", "replace"))
        self.ws_bytes = int(self.lib.mxm_samples_workspace_bytes(self.n_tiles, self.n_entries, self.n_haps))
        self.ws = device_empty((self.ws_bytes // 8 + 1,), torch.float64, self.dev, "the batched loop's workspace")

    def em_iter(self, props, state, colsum):
        """Enqueue one pass for every unfinished entry (mxm_em_iter_samples): colsum[s] <- entry s's unscaled sums."""
        _lib.check(self.lib.mxm_em_iter_samples(ctypes.byref(self.coded), self.row0_ptr, self.n_entries, self.wts.data_ptr(),
                                                props.data_ptr(), self.n_haps, ptr(state), colsum.data_ptr(),
                                                self.ws.data_ptr(), self.ws_bytes, current_stream()), "mxm_em_iter_samples")

    def em_loop(self, inits, tolerance, max_iter, check_every=16):
        """em_loop for every entry at once: inits [S][H] linear.  Returns (ln_cur, ln_new, [(done, iters, l1)])."""
        ln0, p0 = log_inits(inits)
        if ln0.shape != (self.n_entries, self.n_haps):
            raise ValueError("inits must be [%d][%d]" % (self.n_entries, self.n_haps))
        props_cur = torch.from_numpy(p0).to(self.dev)
        ln_cur = torch.from_numpy(ln0).to(self.dev)
        ln_new = ln_cur.clone()
        colsum = torch.zeros_like(props_cur)
        state = new_state(self.n_entries, self.dev)
        host_state = (_lib.EmState * self.n_entries)()
        _lib.check(self.lib.mxm_em_loop_samples(ctypes.byref(self.coded), self.row0_ptr, self.n_entries, self.wts.data_ptr(),
                                                self.n_haps, props_cur.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(),
                                                colsum.data_ptr(), state.data_ptr(), float(tolerance), int(max_iter),
                                                int(check_every), self.ws.data_ptr(), self.ws_bytes, current_stream(),
                                                host_state), "mxm_em_loop_samples")
        return ln_cur, ln_new, [(s.done, s.iters, s.l1) for s in host_state]

    def em_loop_device(self, ln0, p0, tolerance, max_iter, check_every=16):
        """em_loop from a start that is on the device already: ln0 / p0 [S][H] as log_inits forms them (both are taken
        over and updated in place).  Returns (ln_cur, ln_new, the states ON THE DEVICE, [(done, iters, l1)]); nothing
        H-sized crosses the bus (assign.detect_many's entries share a few starts)."""
        if tuple(ln0.shape) != (self.n_entries, self.n_haps) or tuple(p0.shape) != (self.n_entries, self.n_haps):
            raise ValueError("the start must be [%d][%d]" % (self.n_entries, self.n_haps))
        props_cur, ln_cur = p0.contiguous(), ln0.contiguous()
        ln_new = ln_cur.clone()
        colsum = torch.zeros_like(props_cur)
        state = new_state(self.n_entries, self.dev)
        host_state = (_lib.EmState * self.n_entries)()
        _lib.check(self.lib.mxm_em_loop_samples(ctypes.byref(self.coded), self.row0_ptr, self.n_entries, self.wts.data_ptr(),
                                                self.n_haps, props_cur.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(),
                                                colsum.data_ptr(), state.data_ptr(), float(tolerance), int(max_iter),
                                                int(check_every), self.ws.data_ptr(), self.ws_bytes, current_stream(),
                                                host_state), "mxm_em_loop_samples")
        return ln_cur, ln_new, state, [(s.done, s.iters, s.l1) for s in host_state]


class SampleFinish(object):
    """
    The second half of a cohort run over the rows of many samples back to back in ONE records matrix, as SampleBatch holds
    them (assign.finish_many drives it): the contributor vote (mxm_votes_samples), the column gather
    (mxm_gather_columns_samples), the refinement loop with ONE workgroup per sample (mxm_em_loop_samples_narrow) and the
    read assignment (mxm_assign_reads_samples).  rowmax [R]: the records' row maxima (CodedMatrix.rowmax), for the row
    normaliser of the unrefined assignment.  Every per-sample table is [S][ld] with ld = 4, 8 or 16.
    votes_runs / em_loop_runs / assign_runs are the same stages for samples of B EM runs each (mxm_votes_samples_runs,
    mxm_em_loop_samples_narrow_runs, mxm_assign_reads_samples_runs): per-run tables [S][B][...], the vote and the assignment
    over the runs' posteriors folded in run order (em.py:145-161), one workgroup per (sample, run) in the loop.
    boot_weights / em_loop_boot / boot_summary are the bootstrap of the refinement (mxm_bootstrap_weights,
    mxm_em_loop_samples_narrow_boot, mxm_bootstrap_summary; assign.bootstrap_many drives them): B replicates per sample
    under resampled row weights, one workgroup per (sample, replicate) in the loop.
    """
    KMAX = 16
    LDS_CELLS = 9216                # cells (R_s x ncol) up to which the refinement loops linearise a sample in LDS

    def __init__(self, rec, rec_off, ndist, wts, rowmax, row0, n_haps):
        self.lib = _lib.load()
        self.dev = rec.device
        self.rec, self.rec_off, self.ndist, self.wts = rec, rec_off.contiguous(), ndist.contiguous(), wts.contiguous()
        self.rowmax = None if rowmax is None else rowmax.contiguous()
        self.row0 = numpy.ascontiguousarray(row0, dtype=numpy.int64)
        self.n_entries, self.n_rows, self.n_haps = len(self.row0) - 1, int(self.row0[-1]), int(n_haps)
        if self.rec_off.numel() != self.n_rows or self.ndist.numel() != self.n_rows or self.wts.numel() != self.n_rows:
            raise ValueError("rec_off / ndist / weights do not match row0")
        self.coded = _lib.Coded(self.rec.data_ptr(), self.rec_off.data_ptr(), self.ndist.data_ptr(), self.n_rows,
                                None, 0, None, 0, None, 0)
        self.row0_ptr = self.row0.ctypes.data_as(ctypes.c_void_p)
        self.n_tiles = int(self.lib.mxm_samples_plan(self.row0_ptr, self.n_entries, None, 0, None))
        if self.n_tiles < 0:
            raise ValueError("mxm_samples_plan failed: %s" % self.lib.mxm_last_error().decode("utf-8", "replace"))
        self.ws_bytes = int(self.lib.mxm_samples_finish_workspace_bytes(self.n_tiles, self.n_entries, self.KMAX))
        self.ws = torch.empty(self.ws_bytes // 8 + 2, dtype=torch.float64, device=self.dev)

    @staticmethod
    def _i32(table):
        arr = numpy.ascontiguousarray(table, dtype=numpy.int32)
        return arr, arr.ctypes.data_as(ctypes.c_void_p)

    def votes(self, ln_props, want_lse=False):
        """ln_props [S][H] (host).  Returns (best int32[R] device, votes [S][H], counts [S][H], first [S][H] on the host,
        lse [R] device or None, error flags [S])."""
        n, n_haps = self.n_entries, self.n_haps
        host = numpy.ascontiguousarray(ln_props, dtype=numpy.float64)
        if host.shape != (n, n_haps):
            raise ValueError("ln_props must be [%d][%d]" % (n, n_haps))
        lnp = torch.from_numpy(host).to(self.dev)
        props = torch.from_numpy(numpy.exp(host)).to(self.dev) if want_lse else None
        if want_lse and self.rowmax is None:
            raise ValueError("the row normaliser needs the records' rowmax")
        best = torch.empty(self.n_rows, dtype=torch.int32, device=self.dev)
        votes = torch.empty((n, n_haps), dtype=torch.float64, device=self.dev)
        table = torch.empty((2, n, n_haps), dtype=torch.int64, device=self.dev)      # counts, first-seen rows
        lse = torch.empty(self.n_rows, dtype=torch.float64, device=self.dev) if want_lse else None
        state = new_state(n, self.dev)
        _lib.check(self.lib.mxm_votes_samples(ctypes.byref(self.coded), self.row0_ptr, n, n_haps, self.wts.data_ptr(),
                                              lnp.data_ptr(), ptr(props), ptr(self.rowmax) if want_lse else None,
                                              best.data_ptr(), votes.data_ptr(), table[0].data_ptr(), table[1].data_ptr(),
                                              ptr(lse), state.data_ptr(), self.ws.data_ptr(), self.ws_bytes, current_stream()),
                   "mxm_votes_samples")
        raw = state.cpu().numpy().tobytes()
        errors = [st.error != 0 for st in (_lib.EmState * n).from_buffer_copy(raw)]
        table_h = table.cpu().numpy()
        return best, votes.cpu().numpy(), table_h[0], table_h[1], lse, errors

    def votes_device(self, ln_props):
        """votes() for ln_props [S][H] that is on the device, with NOTHING downloaded: returns (votes [S][H] double, first
        [S][H] int64, the vote's states [S]) as device tensors (mxm_votes_samples; no counts, no row normaliser).  A sample
        with a row that has no usable record has NaN votes and state.error = 1."""
        n, n_haps = self.n_entries, self.n_haps
        if tuple(ln_props.shape) != (n, n_haps) or ln_props.dtype != torch.float64:
            raise ValueError("ln_props must be a float64 [%d][%d] device tensor" % (n, n_haps))
        lnp = ln_props.contiguous()
        best = torch.empty(self.n_rows, dtype=torch.int32, device=self.dev)
        votes = torch.empty((n, n_haps), dtype=torch.float64, device=self.dev)
        first = torch.empty((n, n_haps), dtype=torch.int64, device=self.dev)
        state = new_state(n, self.dev)
        _lib.check(self.lib.mxm_votes_samples(ctypes.byref(self.coded), self.row0_ptr, n, n_haps, self.wts.data_ptr(),
                                              lnp.data_ptr(), None, None, best.data_ptr(), votes.data_ptr(), None,
                                              first.data_ptr(), None, state.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                              current_stream()), "mxm_votes_samples")
        return votes, first, state

    def gather(self, cols, ncol, ld):
        """out[r][i] = M[r][cols[s][i]] (i < ncol[s]; -inf in the pad columns): [R][ld] on the device."""
        cols_h, cols_p = self._i32(cols)
        ncol_h, ncol_p = self._i32(ncol)
        out = device_empty((self.n_rows, ld), torch.float64, self.dev, "the reduced EM matrices")
        _lib.check(self.lib.mxm_gather_columns_samples(ctypes.byref(self.coded), self.row0_ptr, self.n_entries, self.n_haps,
                                                       cols_p, ncol_p, ld, out.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                                       current_stream()), "mxm_gather_columns_samples")
        return out

    def em_loop(self, mat, ld, ncol, inits, tolerance, max_iter, check_every=16):
        """em_loop for every sample's reduced matrix at once, one workgroup per sample: inits[s] = [ncol[s]] linear.
        Returns (ln_cur, ln_new) as [S][ld] numpy arrays and [(done, iters, l1)]."""
        n = self.n_entries
        ncol_h, ncol_p = self._i32(ncol)
        p0 = numpy.zeros((n, ld), dtype=numpy.float64)
        for s in range(n):
            p0[s, :ncol_h[s]] = numpy.asarray(inits[s], dtype=numpy.float64).reshape(-1)
        ln0, p0 = log_inits(p0)
        props_cur = torch.from_numpy(p0).to(self.dev)
        ln_cur = torch.from_numpy(ln0).to(self.dev)
        ln_new = ln_cur.clone()
        state = new_state(n, self.dev)
        host_state = (_lib.EmState * n)()
        lin = device_empty((self.n_rows, ld), torch.float64, self.dev, "the linearised reduced matrices")
        _lib.check(self.lib.mxm_em_loop_samples_narrow(ctypes.byref(self.coded), self.row0_ptr, n, self.n_haps, mat.data_ptr(),
                                                       ld, ncol_p, self.wts.data_ptr(), props_cur.data_ptr(), ln_cur.data_ptr(),
                                                       ln_new.data_ptr(), state.data_ptr(), float(tolerance), int(max_iter),
                                                       int(check_every), lin.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                                       current_stream(), host_state), "mxm_em_loop_samples_narrow")
        return ln_cur.cpu().numpy(), ln_new.cpu().numpy(), [(s.done, s.iters, s.l1) for s in host_state]

    def assign(self, mat, ld, ncol, perm, ln_theta, log_props, lse, min_fold, want_post=False):
        """assigned int32[R] (device; contributor ordinal or -1) and, on request, the reduced posterior [R][ld]."""
        n = self.n_entries
        ncol_h, ncol_p = self._i32(ncol)
        perm_h, perm_p = self._i32(perm)
        ln_h = numpy.ascontiguousarray(ln_theta, dtype=numpy.float64)
        ln_d = torch.from_numpy(ln_h).to(self.dev)
        props_d = torch.from_numpy(numpy.exp(ln_h)).to(self.dev)
        lp_d = torch.from_numpy(numpy.ascontiguousarray(log_props, dtype=numpy.float64)).to(self.dev)
        assigned = torch.empty(self.n_rows, dtype=torch.int32, device=self.dev)
        post = device_empty((self.n_rows, ld), torch.float64, self.dev, "the reduced posteriors") if want_post else None
        _lib.check(self.lib.mxm_assign_reads_samples(ctypes.byref(self.coded), self.row0_ptr, n, self.n_haps, mat.data_ptr(), ld,
                                                     ncol_p, perm_p, ln_d.data_ptr(), props_d.data_ptr(), lp_d.data_ptr(),
                                                     ptr(lse), float(numpy.log(min_fold)), assigned.data_ptr(), ptr(post),
                                                     self.ws.data_ptr(), self.ws_bytes, current_stream()),
                   "mxm_assign_reads_samples")
        return assigned, post

    # ---- samples of several EM runs each (include/mixemt_hip_samples_runs.h): every per-run table is [S][B][...] ----
    def _runs_ws(self, n_runs, ld):
        """The workspace for B runs per sample (mxm_samples_runs_workspace_bytes): the object's own, grown if need be."""
        need = int(self.lib.mxm_samples_runs_workspace_bytes(self.n_tiles, self.n_entries, n_runs, ld))
        if need == 0:
            raise ValueError("the batched second half takes 2 .. 64 runs per sample, not %d" % n_runs)
        if need > self.ws_bytes:
            self.ws_bytes = need
            self.ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=self.dev)
        return need

    def votes_runs(self, ln_props, want_lse=False):
        """votes() over the FOLDED posterior of B runs per sample (em.py:145-161): ln_props [S][B][H] (host).  Returns
        (best int32[R] device, votes [S][H], counts [S][H], first [S][H] on the host, lse [R][B] device or None, error
        flags [S])."""
        n, n_haps = self.n_entries, self.n_haps
        host = numpy.ascontiguousarray(ln_props, dtype=numpy.float64)
        if host.ndim != 3 or host.shape[0] != n or host.shape[2] != n_haps:
            raise ValueError("ln_props must be [%d][B][%d]" % (n, n_haps))
        n_runs = host.shape[1]
        if self.rowmax is None:
            raise ValueError("the row normaliser needs the records' rowmax")
        ws_bytes = self._runs_ws(n_runs, 0)
        lnp = torch.from_numpy(host).to(self.dev)
        props = torch.from_numpy(numpy.exp(host)).to(self.dev)
        best = torch.empty(self.n_rows, dtype=torch.int32, device=self.dev)
        votes = torch.empty((n, n_haps), dtype=torch.float64, device=self.dev)
        table = torch.empty((2, n, n_haps), dtype=torch.int64, device=self.dev)      # counts, first-seen rows
        lse = torch.empty((self.n_rows, n_runs), dtype=torch.float64, device=self.dev) if want_lse else None
        state = new_state(n, self.dev)
        _lib.check(self.lib.mxm_votes_samples_runs(ctypes.byref(self.coded), self.row0_ptr, n, n_haps, n_runs,
                                                   self.wts.data_ptr(), lnp.data_ptr(), props.data_ptr(), self.rowmax.data_ptr(),
                                                   best.data_ptr(), votes.data_ptr(), table[0].data_ptr(), table[1].data_ptr(),
                                                   ptr(lse), state.data_ptr(), self.ws.data_ptr(), ws_bytes, current_stream()),
                   "mxm_votes_samples_runs")
        raw = state.cpu().numpy().tobytes()
        errors = [st.error != 0 for st in (_lib.EmState * n).from_buffer_copy(raw)]
        table_h = table.cpu().numpy()
        return best, votes.cpu().numpy(), table_h[0], table_h[1], lse, errors

    def em_loop_runs(self, mat, ld, ncol, inits, tolerance, max_iter, check_every=16):
        """em_loop with B runs per sample, one workgroup per (sample, run): inits[s] = [B][ncol[s]] linear.  Returns
        (ln_cur, ln_new) as [S][B][ld] numpy arrays and [(done, iters, l1)] per sample, one list of B each."""
        n = self.n_entries
        ncol_h, ncol_p = self._i32(ncol)
        n_runs = numpy.atleast_2d(numpy.asarray(inits[0])).shape[0]
        p0 = numpy.zeros((n, n_runs, ld), dtype=numpy.float64)
        for s in range(n):
            p0[s, :, :ncol_h[s]] = numpy.asarray(inits[s], dtype=numpy.float64).reshape(n_runs, ncol_h[s])
        ln0, p0 = log_inits(p0.reshape(n * n_runs, ld))
        ws_bytes = self._runs_ws(n_runs, ld)
        props_cur = torch.from_numpy(p0).to(self.dev)
        ln_cur = torch.from_numpy(ln0).to(self.dev)
        ln_new = ln_cur.clone()
        state = new_state(n * n_runs, self.dev)
        host_state = (_lib.EmState * (n * n_runs))()
        spills = any(int(self.row0[s + 1] - self.row0[s]) * int(ncol_h[s]) > self.LDS_CELLS for s in range(n))
        lin = device_empty((self.n_rows, ld), torch.float64, self.dev, "the linearised reduced matrices") if spills else None
        _lib.check(self.lib.mxm_em_loop_samples_narrow_runs(ctypes.byref(self.coded), self.row0_ptr, n, self.n_haps, n_runs,
                                                            mat.data_ptr(), ld, ncol_p, self.wts.data_ptr(), props_cur.data_ptr(),
                                                            ln_cur.data_ptr(), ln_new.data_ptr(), state.data_ptr(),
                                                            float(tolerance), int(max_iter), int(check_every), ptr(lin),
                                                            self.ws.data_ptr(), ws_bytes, current_stream(), host_state),
                   "mxm_em_loop_samples_narrow_runs")
        states = [(st.done, st.iters, st.l1) for st in host_state]
        return (ln_cur.cpu().numpy().reshape(n, n_runs, ld), ln_new.cpu().numpy().reshape(n, n_runs, ld),
                [states[s * n_runs:(s + 1) * n_runs] for s in range(n)])

    def assign_runs(self, mat, ld, ncol, perm, ln_theta, log_props, lse, min_fold, want_post=False):
        """assign() under the folded reduced posterior of B runs: ln_theta [S][B][ld] (log theta_k per run), log_props
        [S][ld] (the log of the FOLDED proportions), lse [R][B] device or None."""
        n = self.n_entries
        ncol_h, ncol_p = self._i32(ncol)
        perm_h, perm_p = self._i32(perm)
        ln_h = numpy.ascontiguousarray(ln_theta, dtype=numpy.float64)
        if ln_h.ndim != 3 or ln_h.shape[0] != n or ln_h.shape[2] != ld:
            raise ValueError("ln_theta must be [%d][B][%d]" % (n, ld))
        n_runs = ln_h.shape[1]
        if lse is not None and tuple(lse.shape) != (self.n_rows, n_runs):
            raise ValueError("lse must be [%d][%d]" % (self.n_rows, n_runs))
        ws_bytes = self._runs_ws(n_runs, ld)
        lse_d = None if lse is None else lse.contiguous()
        ln_d = torch.from_numpy(ln_h).to(self.dev)
        props_d = torch.from_numpy(numpy.exp(ln_h)).to(self.dev)
        lp_d = torch.from_numpy(numpy.ascontiguousarray(log_props, dtype=numpy.float64)).to(self.dev)
        assigned = torch.empty(self.n_rows, dtype=torch.int32, device=self.dev)
        post = device_empty((self.n_rows, ld), torch.float64, self.dev, "the reduced posteriors") if want_post else None
        _lib.check(self.lib.mxm_assign_reads_samples_runs(ctypes.byref(self.coded), self.row0_ptr, n, self.n_haps, n_runs,
                                                          mat.data_ptr(), ld, ncol_p, perm_p, ln_d.data_ptr(), props_d.data_ptr(),
                                                          lp_d.data_ptr(), ptr(lse_d),
                                                          float(numpy.log(min_fold)), assigned.data_ptr(), ptr(post),
                                                          self.ws.data_ptr(), ws_bytes, current_stream()),
                   "mxm_assign_reads_samples_runs")
        return assigned, post

    # ---- bootstrap replicates of the refinement (include/mixemt_hip_bootstrap.h): per-replicate tables are [S][B][...] ----
    def _boot_ws(self, n_boot, ld):
        """The workspace for B replicates per sample (mxm_bootstrap_workspace_bytes): the object's own, grown if need be."""
        need = int(self.lib.mxm_bootstrap_workspace_bytes(self.n_tiles, self.n_entries, n_boot, ld))
        if need == 0:
            raise ValueError("the bootstrap takes 2 .. 4096 replicates per sample, not %d" % n_boot)
        if need > self.ws_bytes:
            self.ws_bytes = need
            self.ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=self.dev)
        return need

    def boot_weights(self, n_boot, seed, sample_ids):
        """The multinomial resamples of the samples' weights (mxm_bootstrap_weights): wb [R * B] on the device, entry
        B * row0[s] + b * R_s + i, and the samples' error codes [S] (0 fine; 1 a weight that is no non-negative integer;
        2 a total of 0 or of 2^31 and more -- such a sample's wb is NaN)."""
        n = self.n_entries
        ids = numpy.ascontiguousarray(sample_ids, dtype=numpy.uint32)
        if ids.shape != (n,):
            raise ValueError("sample_ids must hold %d ids" % n)
        ws_bytes = self._boot_ws(n_boot, 0)
        wb = device_empty((self.n_rows * n_boot,), torch.float64, self.dev, "the replicates' weights")
        state = new_state(n, self.dev)
        _lib.check(self.lib.mxm_bootstrap_weights(ctypes.byref(self.coded), self.row0_ptr, n, n_boot, self.wts.data_ptr(),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, ids.ctypes.data_as(ctypes.c_void_p),
                                                  wb.data_ptr(), state.data_ptr(), self.ws.data_ptr(), ws_bytes,
                                                  current_stream()), "mxm_bootstrap_weights")
        raw = state.cpu().numpy().tobytes()
        return wb, [int(st.error) for st in (_lib.EmState * n).from_buffer_copy(raw)]

    def em_loop_boot(self, mat, ld, ncol, wb, n_boot, inits, tolerance, max_iter, check_every=16):
        """em_loop under every replicate's weights, one workgroup per (sample, replicate) (mxm_em_loop_samples_narrow_boot):
        inits[s] = [ncol[s]] linear, the start of ALL the sample's replicates.  Returns (ln_cur, ln_new) [S * B][ld] and the
        states [S * B] ON THE DEVICE (boot_summary reads them there), props_cur likewise, and [(done, iters, l1)] per
        sample, one list of B each."""
        n = self.n_entries
        ncol_h, ncol_p = self._i32(ncol)
        p0 = numpy.zeros((n, n_boot, ld), dtype=numpy.float64)
        for s in range(n):
            p0[s, :, :ncol_h[s]] = numpy.asarray(inits[s], dtype=numpy.float64).reshape(1, ncol_h[s])
        ln0, p0 = log_inits(p0.reshape(n * n_boot, ld))
        ws_bytes = self._boot_ws(n_boot, ld)
        props_cur = torch.from_numpy(p0).to(self.dev)
        ln_cur = torch.from_numpy(ln0).to(self.dev)
        ln_new = ln_cur.clone()
        state = new_state(n * n_boot, self.dev)
        host_state = (_lib.EmState * (n * n_boot))()
        spills = any(int(self.row0[s + 1] - self.row0[s]) * int(ncol_h[s]) > self.LDS_CELLS for s in range(n))
        lin = device_empty((self.n_rows, ld), torch.float64, self.dev, "the linearised reduced matrices") if spills else None
        _lib.check(self.lib.mxm_em_loop_samples_narrow_boot(ctypes.byref(self.coded), self.row0_ptr, n, self.n_haps, n_boot,
                                                            mat.data_ptr(), ld, ncol_p, wb.data_ptr(), props_cur.data_ptr(),
                                                            ln_cur.data_ptr(), ln_new.data_ptr(), state.data_ptr(),
                                                            float(tolerance), int(max_iter), int(check_every), ptr(lin),
                                                            self.ws.data_ptr(), ws_bytes, current_stream(), host_state),
                   "mxm_em_loop_samples_narrow_boot")
        states = [(st.done, st.iters, st.l1) for st in host_state]
        return ln_cur, ln_new, props_cur, state, [states[s * n_boot:(s + 1) * n_boot] for s in range(n)]

    def boot_summary(self, n_boot, ld, ncol, ln_new, state, q_lo, q_hi):
        """The replicates' proportions and their summary per (sample, column) (mxm_bootstrap_summary): ln_new [S * B][ld]
        and state [S * B] on the device, as em_loop_boot returns them.  Returns numpy arrays: x [S][B][ld] (pad columns
        0), lo / hi / mean / sd [S][ld] (pad columns NaN) and flag [S] (a replicate of the sample was not usable)."""
        n = self.n_entries
        ncol_h, ncol_p = self._i32(ncol)
        x = torch.zeros((n, n_boot, ld), dtype=torch.float64, device=self.dev)
        table = torch.full((4, n, ld), float("nan"), dtype=torch.float64, device=self.dev)
        flag = torch.zeros(n, dtype=torch.int32, device=self.dev)
        _lib.check(self.lib.mxm_bootstrap_summary(n, n_boot, ld, ncol_p, ln_new.data_ptr(), state.data_ptr(), float(q_lo),
                                                  float(q_hi), x.data_ptr(), table[0].data_ptr(), table[1].data_ptr(),
                                                  table[2].data_ptr(), table[3].data_ptr(), flag.data_ptr(), current_stream()),
                   "mxm_bootstrap_summary")
        table_h = table.cpu().numpy()
        return x.cpu().numpy(), table_h[0], table_h[1], table_h[2], table_h[3], flag.cpu().numpy()

    # ---- nested-model fits over column masks (include/mixemt_hip_support.h): per-fit tables are [S][B][...] ----
    def _support_ws(self, n_fits, ld):
        """The workspace for B fits per sample (mxm_support_workspace_bytes): the object's own, grown if need be."""
        need = int(self.lib.mxm_support_workspace_bytes(self.n_tiles, self.n_entries, n_fits, ld))
        if need == 0:
            raise ValueError("the support fits take 1 .. 256 fits per sample, not %d" % n_fits)
        if need > self.ws_bytes:
            self.ws_bytes = need
            self.ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=self.dev)
        return need

    def _masks(self, masks):
        arr = numpy.ascontiguousarray(masks, dtype=numpy.uint32)
        if arr.ndim != 2 or arr.shape[0] != self.n_entries:
            raise ValueError("masks must be [%d][B]" % self.n_entries)
        return arr, arr.ctypes.data_as(ctypes.c_void_p)

    def em_loop_masks(self, mat, ld, ncol, masks, inits, tolerance, max_iter, check_every=16):
        """em_loop over SUBSETS of every sample's columns, one workgroup per (sample, fit)
        (mxm_em_loop_samples_narrow_masks): masks [S][B] uint32 (bit k = column k of the reduced matrix; 0 = an unused slot,
        left alone), inits[s] = [B][ncol[s]] linear (only the masked-in entries count).  Returns (ln_cur, ln_new) as
        [S][B][ld] numpy arrays -- -inf in a masked-out column -- and [(done, iters, l1)] per sample, one list of B each."""
        n = self.n_entries
        ncol_h, ncol_p = self._i32(ncol)
        mask_h, mask_p = self._masks(masks)
        n_fits = mask_h.shape[1]
        p0 = numpy.zeros((n, n_fits, ld), dtype=numpy.float64)
        for s in range(n):
            p0[s, :, :ncol_h[s]] = numpy.asarray(inits[s], dtype=numpy.float64).reshape(n_fits, ncol_h[s])
        p0 *= ((mask_h[:, :, None] >> numpy.arange(ld, dtype=numpy.uint32)[None, None, :]) & 1)
        ln0, p0 = log_inits(p0.reshape(n * n_fits, ld))
        ws_bytes = self._support_ws(n_fits, ld)
        props_cur = torch.from_numpy(p0).to(self.dev)
        ln_cur = torch.from_numpy(ln0).to(self.dev)
        ln_new = ln_cur.clone()
        state = new_state(n * n_fits, self.dev)
        host_state = (_lib.EmState * (n * n_fits))()
        spills = any(int(self.row0[s + 1] - self.row0[s]) * int(ncol_h[s]) > self.LDS_CELLS for s in range(n))
        lin = device_empty((n_fits * self.n_rows, ld), torch.float64, self.dev, "the fits' linearised matrices") if spills else None
        _lib.check(self.lib.mxm_em_loop_samples_narrow_masks(ctypes.byref(self.coded), self.row0_ptr, n, self.n_haps, n_fits,
                                                             mat.data_ptr(), ld, ncol_p, mask_p, self.wts.data_ptr(),
                                                             props_cur.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(),
                                                             state.data_ptr(), float(tolerance), int(max_iter), int(check_every),
                                                             ptr(lin), self.ws.data_ptr(), ws_bytes, current_stream(), host_state),
                   "mxm_em_loop_samples_narrow_masks")
        states = [(st.done, st.iters, st.l1) for st in host_state]
        return (ln_cur.cpu().numpy().reshape(n, n_fits, ld), ln_new.cpu().numpy().reshape(n, n_fits, ld),
                [states[s * n_fits:(s + 1) * n_fits] for s in range(n)])

    def loglik_masks(self, mat, ld, ncol, masks, ln_props):
        """The fits' log-likelihoods (mxm_loglik_samples_masks): ll[s][b] = sum_r w_r log sum_{k in mask} p_k exp(M_rk) with
        p = exp(ln_props[s][b]) (ln_props [S][B][ld], host or device), and n_eff[s] = sum of w.  Returns numpy arrays
        ll [S][B] (NaN in an unused slot) and n_eff [S]."""
        n = self.n_entries
        ncol_h, ncol_p = self._i32(ncol)
        mask_h, mask_p = self._masks(masks)
        n_fits = mask_h.shape[1]
        if isinstance(ln_props, torch.Tensor):
            lnp = ln_props.to(self.dev, torch.float64).contiguous()
        else:
            lnp = torch.from_numpy(numpy.ascontiguousarray(ln_props, dtype=numpy.float64)).to(self.dev)
        if lnp.numel() != n * n_fits * ld:
            raise ValueError("ln_props must be [%d][%d][%d]" % (n, n_fits, ld))
        ws_bytes = self._support_ws(n_fits, ld)
        ll = torch.full((n, n_fits), float("nan"), dtype=torch.float64, device=self.dev)
        n_eff = torch.empty(n, dtype=torch.float64, device=self.dev)
        _lib.check(self.lib.mxm_loglik_samples_masks(ctypes.byref(self.coded), self.row0_ptr, n, self.n_haps, n_fits,
                                                     mat.data_ptr(), ld, ncol_p, mask_p, self.wts.data_ptr(), lnp.data_ptr(),
                                                     ll.data_ptr(), n_eff.data_ptr(), self.ws.data_ptr(), ws_bytes,
                                                     current_stream()), "mxm_loglik_samples_masks")
        return ll.cpu().numpy(), n_eff.cpu().numpy()


def _fold_runs(ln_next):
    """collect_result's proportions: exp(mean of the runs' LOG proportions), in run order (em.py:155, :163)."""
    res = ln_next[0].copy()
    for run in range(1, len(ln_next)):
        res += ln_next[run]
    if len(ln_next) > 1:
        res /= len(ln_next)
    return numpy.exp(res)


def draw_inits_many(n_samples, n_haps, n_multi=1, alpha=1.0):
    """run_em_many's initial proportions: init_props (em.py:23-36, :123) from numpy's global legacy stream, sample after
    sample, n_multi draws each -- the order a Python loop of run_em over the samples consumes the stream in.  A list of
    [n_multi][H] arrays."""
    return [numpy.stack([init_props(n_haps, alpha=alpha) for _ in range(n_multi)]) for _ in range(n_samples)]


def run_em_many(samples, args, inits=None, tables=None):
    """
    run_em's loop (em.py:94-165) for MANY samples in one batched device pass (mxm_em_loop_samples) instead of a Python
    loop of run_em_ex over them -- opt-in; run_em / run_em_ex are unchanged.
    samples: a list of (matrix, weights), every matrix over the same haplogroups, ALL of one kind:
        (row_ptr, site, obs)    a sample's CSR observations; `tables` (preprocess.HapVarTables) is then required and the
                                rows of all samples are built as records in ONE call (preprocess.build_em_records_many)
        preprocess.CodedMatrix  records; all samples must share one record buffer (views of one build:
                                cm.rows(lo, hi) of build_em_records_many's matrix)
        a dense [R][H] matrix   (numpy or device) encoded with the others in one mxm_encode_rows call
    Returns one dict per sample: props ([H], theta_{k+1} folded over the restarts as run_em folds them), ln_theta_k
    ([n_multi][H], log theta_k), run_props ([n_multi][H]; batch route: also their logs, ln_theta_next), iters / done / l1
    (per restart), inits, and route: "batch", or
    "single" for a sample with rows the encoder left without a record (more than 1024 distinct values: none from
    build_em_matrix) -- that one runs through run_em_ex on its own.
    args.tolerance / max_iter / init_alpha hold for the whole batch.  args.n_multi > 1: every sample takes n_multi
    entries of the batch over the SAME records (offsets repeated, not copied).
    inits: None = drawn as run_em draws them, from numpy's global legacy stream, sample after sample (n_multi draws
    each): sample s alone at the same position of the stream reproduces its own draw; or a list with inits[s] [H] or
    [n_multi][H].
    The second half -- votes, contributors, refinement and read assignment of every sample -- is assign.finish_many
    over these results, batched likewise.  Not here: the posterior matrix (per sample: run_em_ex(records=...)), the quad
    dictionary, several GPUs, fp32 storage.
    """
    from . import preprocess
    lib = _lib.load()
    dev = require_gpu()
    n_multi = int(args.n_multi)
    if not samples or n_multi < 1:
        raise ValueError("run_em_many: no samples")
    mats = [m for m, _ in samples]
    # ---- one records matrix over all samples ----
    single_input = [None] * len(samples)               # what run_em_ex gets if the sample has to run on its own
    if all(isinstance(m, preprocess.CodedMatrix) for m in mats):
        if any(m.rec.data_ptr() != mats[0].rec.data_ptr() for m in mats):
            raise ValueError("run_em_many: records of different builds cannot share a batch (build them with "
                             "preprocess.build_em_records_many)")
        n_haps, rec = mats[0].n_haps, mats[0].rec
        rec_off, ndist = torch.cat([m.rec_off for m in mats]), torch.cat([m.ndist for m in mats])
        counts = [m.n_rows for m in mats]
        single_input = [dict(read_hap_mat=None, records=m) for m in mats]
    elif all(isinstance(m, (tuple, list)) and len(m) == 3 for m in mats):
        if tables is None:
            raise ValueError("run_em_many: CSR samples need tables=")
        cm, row0 = preprocess.build_em_records_many(tables, mats)
        n_haps, rec, rec_off, ndist = cm.n_haps, cm.rec, cm.rec_off, cm.ndist
        counts = list(numpy.diff(row0))
        single_input = [dict(read_hap_mat=None, records=cm.rows(row0[i], row0[i + 1])) for i in range(len(mats))]
    elif not any(isinstance(m, (tuple, list, preprocess.CodedMatrix)) for m in mats):
        dense = [as_device(m, torch.float64, dev) for m in mats]
        if any(d.dim() != 2 or d.shape[1] != dense[0].shape[1] or d.shape[0] < 1 for d in dense):
            raise ValueError("run_em_many: every sample needs a 2-D matrix of at least one row over the same haplogroups")
        n_haps = int(dense[0].shape[1])
        counts = [int(d.shape[0]) for d in dense]
        if not lib.mxm_linear_supported(n_haps):
            raise ValueError("run_em_many: records need H in [65, 8192]")
        plan = EmPlan(torch.cat(dense), numpy.ones(sum(counts)), storage="coded", keep_log_matrix=False)
        rec, rec_off, ndist = plan._coded_keep[:3]
        single_input = [dict(read_hap_mat=d, storage="coded") for d in dense]
    else:
        raise ValueError("run_em_many: the samples must be all CSR triples, all CodedMatrix or all dense matrices")
    wts = [as_device(w, torch.float64, dev).reshape(-1) for _, w in samples]
    if any(int(w.numel()) != int(n) for w, n in zip(wts, counts)):
        raise ValueError("run_em_many: weights do not match the samples' rows")
    # ---- initial proportions: run_em's draws, sample after sample ----
    if inits is None:
        inits = draw_inits_many(len(samples), n_haps, n_multi, args.init_alpha)
    inits = [numpy.ascontiguousarray(numpy.atleast_2d(numpy.asarray(i, dtype=numpy.float64))) for i in inits]
    if len(inits) != len(samples) or any(i.shape != (n_multi, n_haps) for i in inits):
        raise ValueError("run_em_many: inits[s] must be [n_multi][H] for every sample")
    # ---- samples with rows the encoder left dense run on their own ----
    nd_h = ndist.cpu().numpy()
    starts = numpy.concatenate([[0], numpy.cumsum(counts)]).astype(numpy.int64)
    alone = [bool((nd_h[starts[i]:starts[i + 1]] <= 0).any()) for i in range(len(samples))]
    results = [None] * len(samples)
    batch_ids = [i for i in range(len(samples)) if not alone[i]]
    if batch_ids:
        def rows_of(x, i):
            return x[int(starts[i]):int(starts[i + 1])]
        whole = len(batch_ids) == len(samples) and n_multi == 1
        b_off = rec_off if whole else torch.cat([rows_of(rec_off, i) for i in batch_ids for _ in range(n_multi)])
        b_nd = ndist if whole else torch.cat([rows_of(ndist, i) for i in batch_ids for _ in range(n_multi)])
        b_w = torch.cat([wts[i] for i in batch_ids for _ in range(n_multi)])
        row0 = numpy.concatenate([[0], numpy.cumsum([counts[i] for i in batch_ids for _ in range(n_multi)])])
        batch = SampleBatch(rec, b_off, b_nd, b_w, row0, n_haps)
        ln_cur, ln_new, states = batch.em_loop(numpy.concatenate([inits[i] for i in batch_ids]), args.tolerance, args.max_iter)
        ln_k, ln_next = ln_cur.cpu().numpy(), ln_new.cpu().numpy()
        for j, i in enumerate(batch_ids):
            sl = slice(j * n_multi, (j + 1) * n_multi)
            results[i] = {"props": _fold_runs(ln_next[sl]), "ln_theta_k": ln_k[sl].copy(), "ln_theta_next": ln_next[sl].copy(),
                          "run_props": numpy.exp(ln_next[sl]),
                          "iters": [st[1] for st in states[sl]], "done": [st[0] for st in states[sl]],
                          "l1": [st[2] for st in states[sl]], "inits": inits[i], "route": "batch"}
    for i in range(len(samples)):
        if alone[i]:
            res = run_em_ex(weights=samples[i][1], args=args, inits=inits[i], want_read_mix=False, **single_input[i])
            res["route"] = "single"
            results[i] = res
    return results


def run_em(read_hap_mat, weights, args):
    """
    Drop-in for mixemt.em.run_em (em.py:94-165): returns (props, read_mix) --
    linear proportions [H] (numpy) and the log posterior matrix [R][H]
    (numpy if the input was numpy, else a device tensor).
    """
    res = run_em_ex(read_hap_mat, weights, args)
    read_mix = res["read_mix"]
    if not isinstance(read_hap_mat, torch.Tensor):
        read_mix = to_host(read_mix)
    return res["props"], read_mix
