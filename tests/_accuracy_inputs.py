"""
Inputs of the accuracy tests (tests/test_exact_ref.py on the CPU, tests/test_gpu_accuracy.py on the device): small, but
where kernels go wrong.  Everything comes from oracle/, mixemt_amd.synth and numpy.

  * matrices up to H = 5408: REAL rows -- c_oracle.build_em_matrix over a sub-tree of Build 17 (haps[300:300 + H]; all of
    Build 17 at 5408) on synth_reads (700 rows of 150 bp, three more of 4000 bp: rows beyond 1024 distinct values at
    full width -- the dense rest of a records plan; 400-bp rows hold about a hundred -- all drawn from contributor 0, the
    haplogroup that holds 0.6 in the skewed vector: a converged state explains its rows) and synth_pairs (257 merged
    fragments: rows of several hundred distinct values, wide records), contributors (0, H // 2, H - 1);
  * wider than Build 17 (8192, 8200) and H <= 64: the few-values-per-row matrices of
    test_gpu_coded.py::test_shapes_and_ragged_ends;
  * weights: integers 1 .. 4 plus one zero weight;
  * two proportion vectors per matrix: "dirichlet" = rng.dirichlet([1] * H), and "skewed", the converged regime:
    ln p ~ U(-250, -5), then ln p[[0, H // 2]] = log([0.6, 0.3]) and ln p[H - 1] = log(1e-12).  Nothing is normalised:
    the kernels take any positive vector, and so does the reference;
  * the LOOP tests (tests/test_exact_traj.py, tests/test_gpu_accuracy_loops.py): 96-row matrices (loop_matrix) and a third
    vector, "deep" (deep_vector): ln p ~ U(-760, -690) around the skewed vector's three entries, i.e. proportions that are
    subnormal or zero in linear space;
  * the INSTANCE sweep (tests/test_gpu_instances.py, tests/test_exact_ref.py): at most 64 rows of any width in [65, 8192]
    (edge_rows: column slices of the full-width real rows, few_values beyond Build 17), and few_quads, few_values with every
    value four columns long, for the quad passes beyond Build 17's width.
"""
import numpy

from oracle import c_oracle

N_READS, N_LONG, N_PAIRS, LONG_READ = 700, 3, 257, 4000
_tables = {}
_matrices = {}


def tables_for(b17, n_haps):
    from mixemt_amd import preprocess
    refseq, phy, haps, tables = b17
    if n_haps == len(haps):
        return tables
    if n_haps not in _tables:
        _tables[n_haps] = preprocess.HapVarTables.build(refseq, phy, haps[300:300 + n_haps])
    return _tables[n_haps]


def real_rows(b17, n_haps, kind):
    """kind "reads": 700 rows of 150-bp reads + 3 of 4000-bp reads (the LAST three rows); "pairs": 257 merged fragments.
    The fp64 log matrix with the reference's bits (C oracle), built once per (width, kind) and never written to."""
    from mixemt_amd import synth
    key = (n_haps, kind)
    if key not in _matrices:
        refseq = b17[0]
        tables = tables_for(b17, n_haps)
        contrib = (0, n_haps // 2, n_haps - 1)
        if kind == "reads":
            parts = [synth.synth_reads(tables, len(refseq), N_READS, seed=n_haps, contrib=contrib),
                     synth.synth_reads(tables, len(refseq), N_LONG, seed=n_haps + 1, contrib=contrib, read_len=LONG_READ,
                                       props=(1.0, 0.0, 0.0))]
        else:
            parts = [synth.synth_pairs(tables, len(refseq), N_PAIRS, seed=n_haps, contrib=contrib)]
        mats = [c_oracle.build_em_matrix(tables.expected, tables.lhit, tables.lmiss, row_ptr, site, obs, n_haps)
                for row_ptr, site, obs, _ in parts]
        mat = numpy.ascontiguousarray(numpy.concatenate(mats))
        mat.setflags(write=False)
        _matrices[key] = mat
    return _matrices[key]


def few_values(n_rows, n_haps):
    """test_gpu_coded.py::test_shapes_and_ragged_ends' matrices: at most 40 distinct values per row."""
    key = (n_haps, "few%d" % n_rows)
    if key not in _matrices:
        rng = numpy.random.default_rng(n_rows + n_haps)
        few = rng.normal(-20.0, 6.0, size=(n_rows, 40))
        mat = numpy.take_along_axis(few, rng.integers(0, 40, size=(n_rows, n_haps)), axis=1)
        mat.setflags(write=False)
        _matrices[key] = mat
    return _matrices[key]


def edge_rows(b17, n_haps, n_rows):
    """(label, log matrix [n_rows][n_haps]) of the instance sweep (tests/test_gpu_instances.py, at most 64 rows of ANY
    width): up to Build 17's width the first n_haps columns of real_rows(b17, 5408, ...) -- the sub-tree of the first
    n_haps haplogroups, whose matrix over the same reads is this column slice bit for bit (the variant sites are the
    whole tree's either way) -- from 37 rows on the last four of them merged pairs (rows of several hundred distinct
    values: wide records at full width); beyond it few_values.  Column 0 stays the reads' contributor."""
    if n_haps > 5408 or n_haps < 65:
        return "few values[:%d] %d" % (n_rows, n_haps), numpy.array(few_values(64, n_haps)[:n_rows])
    n_pairs = 4 if n_rows >= 37 else 0
    rows = [real_rows(b17, 5408, "reads")[:n_rows - n_pairs, :n_haps]]
    if n_pairs:
        rows.append(real_rows(b17, 5408, "pairs")[:n_pairs, :n_haps])
    return "reads + pairs[:%d] %d" % (n_rows, n_haps), numpy.ascontiguousarray(numpy.concatenate(rows))


def few_quads(n_rows, n_haps):
    """few_values with every value four columns long: at most 40 distinct aligned quads per row -- every row of it
    gets a quad record, which few_values' rows (40^4 possible quads) never do.  The quad passes beyond Build 17's width."""
    quarter = few_values(n_rows, (n_haps + 3) // 4)
    return numpy.ascontiguousarray(numpy.repeat(quarter, 4, axis=1)[:, :n_haps])


def weights(n_rows, seed=0):
    rng = numpy.random.default_rng(1000 + seed + n_rows)
    wts = rng.integers(1, 5, size=n_rows).astype(numpy.float64)
    if n_rows > 1:
        wts[n_rows // 3] = 0.0
    return wts


def prop_vectors(n_haps, seed=0):
    """{"dirichlet": (props, ln_props), "skewed": (props, ln_props)}: props = exp(ln_props) for the skewed vector and
    ln_props = log(props) for the Dirichlet one, both in fp64 -- the two arrays a kernel may read."""
    rng = numpy.random.default_rng(77 + seed + n_haps)
    p = rng.dirichlet([1.0] * n_haps)
    ln = rng.uniform(-250.0, -5.0, size=n_haps)
    ln[[0, n_haps // 2]] = numpy.log([0.6, 0.3])
    ln[n_haps - 1] = numpy.log(1e-12)
    return {"dirichlet": (p, numpy.log(p)), "skewed": (numpy.exp(ln), ln)}


def deep_vector(n_haps, seed=0, head=(0.6, 0.3)):
    """"deep" (props, ln_props), the regime every long run ends in: ln p ~ U(-760, -690), then the three entries of the
    skewed vector -- about half the proportions are subnormal in fp64 (ln p < -708.4), a fifth are zero (ln p < -745.1),
    and more cross either line while a loop runs (tests/test_exact_traj.py prints the counts).  A generator of its own:
    prop_vectors' draws stay what they were."""
    rng = numpy.random.default_rng(7700 + seed + n_haps)
    ln = rng.uniform(-760.0, -690.0, size=n_haps)
    ln[[0, n_haps // 2]] = numpy.log(head)             # (another head: a restart that takes another way, and stops elsewhere)
    ln[n_haps - 1] = numpy.log(1e-12)
    return numpy.exp(ln), ln


LOOP_ROWS = 96
LOOP_WIDTHS_REAL = (66, 1025, 5408)
LOOP_WIDTHS_LOG = (3, 16, 17, 64, 8200)         # (16: the widest instance of the narrow one-launch loop)
LOOP_STEPS = (2, 3, 10, 40)


def loop_matrix(b17, n_haps):
    """(label, log matrix, weights) of the loop tests: 96 rows -- the first 93 reads and the three 4000-bp rows at the real
    widths (from 63 rows on the one-launch records loop takes Build 17's width itself), few-values rows at the log-space
    widths."""
    if n_haps in LOOP_WIDTHS_REAL:
        reads = real_rows(b17, n_haps, "reads")
        mat, label = numpy.concatenate([reads[:LOOP_ROWS - N_LONG], reads[N_READS:]]), "reads[:93] + long"
    else:
        mat, label = few_values(LOOP_ROWS, n_haps), "few values"
    assert mat.shape == (LOOP_ROWS, n_haps)
    return "%s %d" % (label, n_haps), numpy.array(mat), weights(LOOP_ROWS)


def loop_vectors(n_haps):
    """{name: (props, ln_props)}: the two existing vectors, and "deep" where the width leaves it entries of its own."""
    vecs = dict(prop_vectors(n_haps))
    if n_haps >= 16:
        vecs["deep"] = deep_vector(n_haps)
    return vecs


def linearise(mat):
    """exp(M - rowmax) in fp64 on the host: what the CPU test feeds the reference (the device tests read the device's P)."""
    mat = numpy.asarray(mat)
    return numpy.exp(mat - mat.max(axis=1, keepdims=True))


# (name, width, how to get the log matrix): every matrix the two test modules use
LINEAR_WIDTHS_REAL = (65, 66, 1023, 1024, 1025, 2050, 5408)
LOG_WIDTHS = (1, 2, 17, 64, 8200)


def all_inputs(b17):
    """Every (label, M, w) of section 5, for the CPU test."""
    for n_haps in LINEAR_WIDTHS_REAL:
        reads = real_rows(b17, n_haps, "reads")
        yield "reads %d" % n_haps, reads, weights(len(reads))
        if n_haps in (66, 5408):
            pairs = real_rows(b17, n_haps, "pairs")
            yield "pairs %d" % n_haps, pairs, weights(len(pairs))
    yield "reads[:37] 5408", real_rows(b17, 5408, "reads")[:37], weights(37)
    for n_haps in (8192,) + LOG_WIDTHS:
        mat = few_values(700, n_haps)
        yield "few values %d" % n_haps, mat, weights(700)
