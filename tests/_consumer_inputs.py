"""
Inputs of the consumer accuracy tests (tests/test_exact_consumers.py on the CPU, tests/test_gpu_accuracy_consumers.py on the
device), on top of tests/_accuracy_inputs.py -- the smallest shapes at which each kernel can go wrong; nothing above 400
rows, nothing wider than Build 17.  Both modules take their cases from here, so the CPU module's statements (every honest
fp64 pass inside the rule, at most 1 % undecided rows per decision case from the reference alone) are about the very inputs
the device sees.

  * ORPHAN ROWS: every fourth row of a matrix (r % 4 == 3) is -inf in every column whose "deep" log proportion is >= t, t
    in turn -700, -715, -738, -750 -- supported only by proportions that are small normal numbers whose products with
    P < 1 underflow gradually (-700), subnormal (-715, -738) or zero (-750: the all-underflowed redo the kernels always had);
  * the vote's vectors per run: "skewed" (every run a skewed vector), "mixed" (skewed, deep, skewed: an orphan row's
    normaliser is in the subnormal window in one run and normal in the others), "deep" (every run deep);
  * the assignment's reduced matrices have CONTINUOUS values (rng.normal): a few-values row holds the same value in many
    columns, its top two tie exactly in a third of the rows at 16 columns, and a tie is an undecided row.
"""
import numpy

import _accuracy_inputs as inputs

ORPHAN_T = (-700.0, -715.0, -738.0, -750.0)
VOTE_KINDS = ("skewed", "mixed", "deep")
VOTE_SAMPLES = (1, 63, 64, 65, 200)
VECTOR_WIDTHS = (1, 2, 255, 256, 257, 5408)
FOLD_WIDTHS = (1, 2, 255, 256)
FOLD_INPUTS = (1, 2, 7, 8)
FOLD_ROWS = 5
_made = {}


def with_orphans(mat, ln_deep):
    """A copy of `mat` whose rows r % 4 == 3 are orphans under `ln_deep` (thresholds in turn); -> (matrix, threshold per row
    with NaN for the ordinary rows)."""
    mat = numpy.array(mat)
    t_of = numpy.full(len(mat), numpy.nan)
    for r in range(3, len(mat), 4):
        t = ORPHAN_T[(r // 4) % 4]
        gone = ln_deep >= t
        assert 0 < gone.sum() < len(ln_deep), "an orphan row needs a supported column (t = %g)" % t
        mat[r, gone] = -numpy.inf
        t_of[r] = t
    return mat, t_of


def orphan_matrix(b17, n_haps, kind="few", n_rows=400):
    """(label, log matrix with orphan rows, threshold per row): few-values rows, or the first rows of the merged pairs at
    Build 17's width (wide records).  Made once, never written to."""
    key = (n_haps, kind, n_rows)
    if key not in _made:
        base = inputs.few_values(n_rows, n_haps) if kind == "few" else inputs.real_rows(b17, n_haps, kind)[:n_rows]
        mat, t_of = with_orphans(base, inputs.deep_vector(n_haps)[1])
        mat.setflags(write=False)
        _made[key] = ("%s[:%d] %d + orphans" % (kind, n_rows, n_haps), mat, t_of)
    return _made[key]


def run_vectors(n_haps, kind, n_runs):
    """ln_props [n_runs][H] of the vote / posterior cases."""
    skew = [inputs.prop_vectors(n_haps, seed=b)["skewed"][1] for b in range(3)]
    deep = [inputs.deep_vector(n_haps, seed=b, head=((0.6, 0.3), (0.25, 0.55), (0.5, 0.4))[b])[1] for b in range(3)]
    rows = {"skewed": skew, "mixed": [skew[0], deep[0], skew[1]], "deep": deep}[kind]
    return numpy.ascontiguousarray(numpy.stack(rows[:n_runs]))


def sample_cuts(n_rows):
    """row0 of the vote's samples: 1, 63, 64, 65 and 200 rows as far as the matrix reaches."""
    row0 = [0]
    for n in VOTE_SAMPLES:
        if row0[-1] + n <= n_rows:
            row0.append(row0[-1] + n)
    return numpy.array(row0, dtype=numpy.int64)


def sample_run_vectors(n_haps, kind, n_runs, n_samples):
    """ln_props [S][B][H]: the runs of run_vectors, in REVERSED run order for the odd samples (the fold is taken in run order,
    and a kernel that reads another sample's table gets another result)."""
    runs = run_vectors(n_haps, kind, n_runs)
    return numpy.ascontiguousarray(numpy.stack([runs if s % 2 == 0 else runs[::-1] for s in range(n_samples)]))


def vote_matrices(b17):
    """The two matrices of the vote and posterior cases: byte codes at H = 128, wide records at 5408."""
    return [orphan_matrix(b17, 128, "few", 400), orphan_matrix(b17, 5408, "pairs", 64)]


# ---------------------------------------------------------------- the small vector entries
def vector_pairs(n_haps):
    """{name: (a, b)} of log vectors for mxm_l1_exp_diff: pairs that differ in the last bits and pairs that differ widely,
    from the dirichlet, skewed and deep vectors; "deep, below -745" holds only entries whose exp is exactly 0."""
    vecs = dict(inputs.prop_vectors(n_haps))
    vecs["deep"] = inputs.deep_vector(n_haps)
    rng = numpy.random.default_rng(4100 + n_haps)
    out = {}
    for name, (_, ln) in vecs.items():
        out[name + ", last bits"] = (ln, numpy.nextafter(ln, ln + rng.choice([-1.0, 1.0], size=n_haps)))
        out[name + ", one step of 0.1"] = (ln, ln + rng.normal(0.0, 0.1, size=n_haps))
    out["dirichlet against skewed"] = (vecs["dirichlet"][1], vecs["skewed"][1])
    out["skewed against deep"] = (vecs["skewed"][1], vecs["deep"][1])
    low = rng.uniform(-760.0, -746.0, size=n_haps)
    out["deep, below -745"] = (low, low[::-1].copy())
    return out


def normalize_vectors(n_haps):
    """{name: T} for mxm_log_normalize: the linear dirichlet, skewed and deep vectors times a scale (T is not normalised)."""
    vecs = dict(inputs.prop_vectors(n_haps))
    vecs["deep"] = inputs.deep_vector(n_haps)
    return {name: numpy.ascontiguousarray(props * scale) for (name, (props, _)), scale in zip(vecs.items(), (700.0, 3.0, 1.0))}


# ---------------------------------------------------------------- the fold
def fold_blocks(n_haps, n_in):
    """[acc, in_0 .. in_{n_in - 1}], each [5][H] fp64: posteriors of a few-values matrix under n_in + 1 vectors, then
    row 1 equal in all blocks, row 2 -inf in some, row 3 -inf in all, row 4 more than 745 apart from block to block and
    below -745 in every block (a fold in linear space loses it altogether)."""
    mat = inputs.few_values(FOLD_ROWS, n_haps)
    blocks = []
    for k in range(n_in + 1):
        vec = inputs.prop_vectors(n_haps, seed=k)["skewed" if k % 2 else "dirichlet"][1]
        a = mat + vec[None, :]
        m = a.max(axis=1, keepdims=True)
        blocks.append(a - (m + numpy.log(numpy.exp(a - m).sum(axis=1, keepdims=True))))
    for k, blk in enumerate(blocks):
        blk[1] = blocks[0][1]
        if k % 2 == 1:
            blk[2] = -numpy.inf
        blk[3] = -numpy.inf
        blk[4] = blocks[0][4] - 800.0 * (1 + (k * 3) % 4)
        blk[0, 0] = blocks[0][0, 0]                        # (and one column of an ordinary row equal in all blocks)
    return [numpy.ascontiguousarray(b) for b in blocks]


# ---------------------------------------------------------------- the assignment
def smooth_values(n_rows, n_cols, seed=0):
    rng = numpy.random.default_rng(5200 + seed + 31 * n_rows + n_cols)
    return rng.normal(-20.0, 6.0, size=(n_rows, n_cols))


def dense_assign_case(n_cols, ascending):
    """mxm_assign_reads: X = the fp64 posterior of a continuous 400 x 128 matrix under a skewed vector (bits in, nothing
    else is asked of them), log_props [H], nC columns -- the three columns that hold the mass among them."""
    n_rows, n_haps = 400, 128
    ln = inputs.prop_vectors(n_haps)["skewed"][1]
    a = smooth_values(n_rows, n_haps) + ln[None, :]
    m = a.max(axis=1, keepdims=True)
    X = numpy.ascontiguousarray(a - (m + numpy.log(numpy.exp(a - m).sum(axis=1, keepdims=True))))
    rng = numpy.random.default_rng(n_cols)
    others = numpy.setdiff1d(numpy.arange(n_haps), [0, 64, 127])
    cols = numpy.concatenate([[0, 64, 127][:min(n_cols, 3)], rng.choice(others, size=max(n_cols - 3, 0), replace=False)])
    cols = numpy.sort(cols) if ascending else rng.permutation(cols)
    return X, ln, cols.astype(numpy.int32)


ASSIGN_SHAPES = {4: (2, 3), 8: (2, 3), 16: (2, 3, 16)}
ASSIGN_ROWS = (65, 1, 64, 100, 63, 37)


def assign_batch(ld, n_runs):
    """One call of mxm_assign_reads_samples (n_runs = 1) or _runs: per K of ASSIGN_SHAPES[ld] a well-conditioned sample and
    one whose every column is deep.  -> dict: row0, ncol [S], perm [S][ld], M [R][ld] (-inf pads, a few -inf cells),
    ln_theta [S][B][ld], log_props [S][ld], lse [R][B] (a given normaliser: any fp64 numbers >= the internal one), kinds [S].
    Deep samples: column 0 at -752 (its exp is 0), the others in (-744, -700) (subnormal, or normal with products that
    underflow gradually); every tenth row of theirs is -inf outside column 0: the linear sum is then exactly 0."""
    rng = numpy.random.default_rng(100 * ld + n_runs)
    shapes = [(k, kind) for k in ASSIGN_SHAPES[ld] for kind in ("well", "deep")]
    rows = [ASSIGN_ROWS[i % len(ASSIGN_ROWS)] for i in range(len(shapes))]
    row0 = numpy.concatenate([[0], numpy.cumsum(rows)]).astype(numpy.int64)
    n_rows, n = int(row0[-1]), len(shapes)
    M = numpy.full((n_rows, ld), -numpy.inf)
    ln_theta = numpy.full((n, n_runs, ld), -numpy.inf)
    log_props = numpy.full((n, ld), -numpy.inf)
    perm = numpy.zeros((n, ld), dtype=numpy.int32)
    for s, (k, kind) in enumerate(shapes):
        lo, hi = int(row0[s]), int(row0[s + 1])
        block = smooth_values(hi - lo, k, seed=ld + s)
        rest = block[:, 1:]
        rest[rng.random(rest.shape) < 0.02] = -numpy.inf
        if kind == "deep":
            block[9::10, 1:] = -numpy.inf
        M[lo:hi, :k] = block
        for b in range(n_runs):
            if kind == "well":
                ln_theta[s, b, :k] = numpy.log(rng.dirichlet([1.0] * k))
            else:
                ln_theta[s, b, :k] = rng.uniform(-744.0, -700.0, size=k)
                ln_theta[s, b, 0] = -752.0
        log_props[s, :k] = ln_theta[s].mean(axis=0)[:k] + rng.normal(0.0, 0.01, size=k)
        perm[s, :k] = rng.permutation(k)
    sample_of = numpy.repeat(numpy.arange(n), rows)
    with numpy.errstate(invalid="ignore"):
        top = numpy.stack([(M + ln_theta[sample_of, b]).max(axis=1) for b in range(n_runs)], axis=1)
    lse = numpy.ascontiguousarray(top + rng.uniform(0.7, 3.0, size=top.shape))
    return {"row0": row0, "ncol": numpy.array([k for k, _ in shapes], dtype=numpy.int32), "perm": perm, "M": M,
            "ln_theta": ln_theta, "log_props": log_props, "lse": lse, "kinds": [kind for _, kind in shapes],
            "sample_of": sample_of}
