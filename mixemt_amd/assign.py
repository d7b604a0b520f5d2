"""
Consumers of the EM result that reduce the [R][H] posterior matrix to one small
value per read -- the "next" rows f-1..f-3 of SURVEY.md section 8.  On the
device they are single streaming / gather passes over a matrix that is already
resident, and they remove the 43 GB device->host copy of `read_mix` the
reference's NumPy versions would need:

    find_contribs_from_reads   <- assemble._find_contribs_from_reads  assemble.py:103-123
    get_contributors (+ _records) <- assemble.get_contributors        assemble.py:31-100
    check_contrib_phy_vars     <- assemble._check_contrib_phy_vars    assemble.py:126-208 (host logic over the pileup of
                                  observe.observe_bases)
    read_votes / report_read_votes <- stats.report_read_votes          stats.py:34-45
    update_contribs            <- assemble.update_contribs             assemble.py:211-230
    assign_read_indexes        <- assemble.assign_read_indexes         assemble.py:284-334
                                  (with _find_best_n_for_read :267-281)
    assign_reads (ContribReads) <- assemble.assign_reads               assemble.py:233-264 (one label per alignment)
                                  (consensus and extension over the labels: mixemt_amd/assemble.py)

Matrices may be numpy arrays (uploaded) or ROCm tensors.
"""

import collections
import collections.abc
import sys

import numpy

from . import _lib
from ._dev import as_device, current_stream, ptr, require_gpu, torch


def _contributors_on_device(best_d, votes_d, n_haps, min_reads):
    """
    Columns with at least min_reads votes in the order their haplogroup first won a row (assemble.py:115-123): the
    first-seen row of every haplogroup is formed on the device (mxm_first_seen), so 2 x H values come back instead of
    best[R] (4 MB and a numpy.unique over R at 10^6 rows: 23 ms for a 1.5 ms pass).
    """
    lib = _lib.load()
    n_rows = best_d.numel()
    first = torch.empty(n_haps, dtype=torch.int64, device=best_d.device)
    _lib.check(lib.mxm_first_seen(best_d.data_ptr(), n_rows, n_haps, first.data_ptr(), current_stream()), "mxm_first_seen")
    first_h, votes_h = first.cpu().numpy(), votes_d.cpu().numpy()
    seen = numpy.flatnonzero(first_h < n_rows)
    order = seen[numpy.argsort(first_h[seen], kind="stable")]
    return [int(h) for h in order if votes_h[h] >= min_reads], order, votes_h


def _row_argmax_votes_device(read_hap_mat, wts):
    lib = _lib.load()
    dev = require_gpu()
    mat = as_device(read_hap_mat, torch.float64, dev)
    n_rows, n_haps = mat.shape
    w_d = None if wts is None else as_device(wts, torch.float64, dev)
    best = torch.empty(n_rows, dtype=torch.int32, device=dev)
    votes = torch.zeros(n_haps, dtype=torch.float64, device=dev)
    if n_rows:
        nbytes = lib.mxm_workspace_bytes(n_rows, n_haps, 1)       # per-workgroup vote rows (no float atomics)
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
        _lib.check(lib.mxm_row_argmax_votes(mat.data_ptr(), mat.stride(0), ptr(w_d), n_rows, n_haps,
                                            best.data_ptr(), votes.data_ptr(), ws.data_ptr(), nbytes,
                                            current_stream()), "mxm_row_argmax_votes")
    return best, votes


def row_argmax_votes(read_hap_mat, wts=None):
    """
    best[r] = first index of the row maximum (numpy.argmax semantics) and
    votes[h] = sum of wts over the rows that picked h (mxm_row_argmax_votes).
    Returns (best int32[R], votes float64[H]) as numpy arrays.
    """
    best, votes = _row_argmax_votes_device(read_hap_mat, wts)
    return best.cpu().numpy(), votes.cpu().numpy()


def row_argmax_votes_records(cm, ln_theta_k, wts=None):
    """
    row_argmax_votes of run_em's returned posterior for a matrix that exists only as records
    (preprocess.CodedMatrix) -- neither the dense matrix nor the posterior matrix is made
    (mxm_row_argmax_votes_coded).  ln_theta_k: the log theta_k of the run ([H]) or of every run of a multi-run
    ([n_multi][H], em.run_em_ex's "ln_theta_k"): the reference votes on the logaddexp fold of the runs' posteriors
    (em.py:156 -> assemble.py:115-123), in which each run's row normaliser weighs that run's columns -- with one
    run it drops out and best = argmax_h (ln_theta[h] + M[r][h]).  Rows without a record are read from their
    dense copies by the same entry point; votes are summed without float atomics.
    Returns (best int32[R], votes float64[H]) as numpy arrays.
    """
    best, votes = _row_argmax_votes_records_device(cm, ln_theta_k, wts)
    return best.cpu().numpy(), votes.cpu().numpy()


def _row_argmax_votes_records_device(cm, ln_theta_k, wts=None):
    import ctypes
    lib = _lib.load()
    dev = cm.rec.device
    if isinstance(ln_theta_k, torch.Tensor):
        lnp = as_device(ln_theta_k, torch.float64, dev)
        lnp = (lnp.reshape(1, -1) if lnp.dim() == 1 else lnp).contiguous()
        props = torch.exp(lnp)
    else:
        # H values per run: exponentiated on the host (the process's first torch.exp on the device loads torch's
        # elementwise kernels -- 18 ms that landed in this 3 ms stage)
        host = numpy.atleast_2d(numpy.ascontiguousarray(ln_theta_k, dtype=numpy.float64))
        lnp = torch.from_numpy(host).to(dev)
        props = torch.from_numpy(numpy.exp(host)).to(dev)
    n_runs = lnp.shape[0]
    if lnp.dim() != 2 or lnp.shape[1] != cm.n_haps:
        raise ValueError("ln_theta_k does not match the matrix width")
    best = torch.zeros(cm.n_rows, dtype=torch.int32, device=dev)
    votes = torch.zeros(cm.n_haps, dtype=torch.float64, device=dev)
    w_d = None if wts is None else as_device(wts, torch.float64, dev)
    nbytes = lib.mxm_workspace_bytes(cm.n_rows, cm.n_haps, 1)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    coded = cm.struct()
    n_rest = int(cm.rest_rows.numel())
    _lib.check(lib.mxm_row_argmax_votes_coded(
        ctypes.byref(coded), cm.n_haps, n_runs, lnp.data_ptr(), props.data_ptr(), cm.rowmax.data_ptr(),
        cm.m_rest.data_ptr() if n_rest else 0, cm.m_rest.stride(0) if n_rest else 0,
        cm.rest_rows.data_ptr() if n_rest else 0, n_rest, ptr(w_d), best.data_ptr(), votes.data_ptr(),
        ws.data_ptr(), nbytes, current_stream()), "mxm_row_argmax_votes_coded")
    return best, votes


def find_contribs_from_records(cm, ln_theta_k, wts, args):
    """find_contribs_from_reads (assemble.py:103-123) from records and the EM's log theta_k ([H], or [n_multi][H]
    for a multi-run: see row_argmax_votes_records)."""
    best, votes = _row_argmax_votes_records_device(cm, ln_theta_k, wts)
    return _contributors_on_device(best, votes, cm.n_haps, args.min_reads)[0]


def vote_table_from_records(cm, ln_theta_k, wts=None):
    """(columns in first-seen order, votes[H]) of the records' vote (stats.py:34-45 / assemble.py:115-123); H-sized
    arrays only leave the device."""
    best, votes = _row_argmax_votes_records_device(cm, ln_theta_k, wts)
    _, order, votes_h = _contributors_on_device(best, votes, cm.n_haps, 0)
    return order, votes_h


def _first_seen_order(best):
    """Column indexes in the order they first appear in `best` (dict insertion order
    of the reference's vote table, assemble.py:116-119)."""
    uniq, first = numpy.unique(best, return_index=True)
    return uniq[numpy.argsort(first, kind="stable")]


def find_contribs_from_reads(read_hap_mat, wts, args):
    """
    Haplogroup columns that are the most probable source of at least
    args.min_reads fragments (assemble.py:103-123), in the reference's order
    (first appearance among the rows).
    """
    best, votes = _row_argmax_votes_device(read_hap_mat, wts)
    return _contributors_on_device(best, votes, votes.numel(), args.min_reads)[0]


def check_contrib_phy_vars(phylo, obs, contrib_prop, args):
    """
    assemble._check_contrib_phy_vars (assemble.py:126-208): from the largest proportion down, a candidate is kept when
    enough of its variants that no kept candidate has already claimed are seen in the sample -- a (pos, derived base)
    is seen when obs.obs_at(pos, der) >= max(args.min_var_reads, obs.total_obs(pos) * args.frac_var_reads); kept when
    it has no such variants, or args.var_count is set and met, or the seen fraction is >= args.var_fraction.  A kept
    candidate's seen variants and its ancestral bases (phylo.get_ancestral) are claimed.  `obs`: an
    observe.ObservedBases (or the reference's).  contrib_prop: [[haplogroup, proportion], ...] by descending proportion.
    Verbose lines go to stderr, as the reference writes them.
    """
    from .phylotree import der_allele, pos_from_var
    used_vars = set()
    ignore_haps = set()
    threshold = 0                                  # (the reference's "Keeping" line prints the last site's threshold)
    if args.verbose:
        sys.stderr.write("Checking diagnostic variants:\n")
    for hap, _ in contrib_prop:
        uniq_vars = set((pos_from_var(var), der_allele(var)) for var in phylo.hap_var[hap])
        uniq_vars -= used_vars
        if args.verbose:
            sys.stderr.write("%s (%d unique variants)\n" % (hap, len(uniq_vars)))
        found_vars = set()
        for pos, der in sorted(uniq_vars):
            seen, total = obs.obs_at(pos, der), obs.total_obs(pos)
            if args.verbose:
                var = "%d%s" % (pos + 1, der)
                sys.stderr.write("  %s: %d/%d\n" % (var.rjust(6), seen, total))
            threshold = max(args.min_var_reads, total * args.frac_var_reads)
            if seen >= threshold:
                found_vars.add((pos, der))
        if (len(uniq_vars) == 0
                or (args.var_count is not None and len(found_vars) >= args.var_count)
                or (float(len(found_vars)) / len(uniq_vars) >= args.var_fraction)):
            if args.verbose:
                sys.stderr.write("Keeping '%s': %d/%d unique variant bases observed at least %d times.\n"
                                 % (hap, len(found_vars), len(uniq_vars), threshold))
            used_vars.update(found_vars)
            used_vars.update(phylo.get_ancestral(hap))
        else:
            if args.verbose:
                sys.stderr.write("Ignoring '%s': only %d/%d unique variant bases observed.\n"
                                 % (hap, len(found_vars), len(uniq_vars)))
            ignore_haps.add(hap)
    return [con for con in contrib_prop if con[0] not in ignore_haps]


def _contributor_table(phylo, obs, haplogroups, props, find, args):
    """assemble.get_contributors (assemble.py:31-100) around a candidate finder `find()` -> column indexes."""
    if not getattr(args, "contributors", None):
        contributors = find()
    else:
        contributors = []
        for con in args.contributors.split(","):
            try:
                contributors.append(haplogroups.index(con))
            except ValueError:
                raise ValueError("Unknown haplogroup '%s'" % (con))
    contrib_prop = [[haplogroups[con], props[con]] for con in contributors]
    contrib_prop.sort(key=lambda con: con[1], reverse=True)
    if args.var_check and not getattr(args, "contributors", None):
        contrib_prop = check_contrib_phy_vars(phylo, obs, contrib_prop, args)
    name_fmt = "hap%%0%dd" % (len(str(len(contrib_prop) + 1)))
    for num, con in enumerate(contrib_prop):
        con.insert(0, name_fmt % (num + 1))
    return contrib_prop


def get_contributors(phylo, obs, haplogroups, wts, em_results, args):
    """
    assemble.get_contributors (assemble.py:31-100): [[hapNN, haplogroup, proportion], ...] by descending proportion --
    the candidates with at least args.min_reads votes (or args.contributors, comma-separated: ValueError for an unknown
    one), filtered by check_contrib_phy_vars when args.var_check and no args.contributors.  em_results = (props,
    read_hap_mat) with the posterior matrix dense (numpy or device).
    """
    props, read_hap_mat = em_results
    return _contributor_table(phylo, obs, haplogroups, props,
                              lambda: find_contribs_from_reads(read_hap_mat, wts, args), args)


def get_contributors_records(phylo, obs, haplogroups, wts, props, cm, ln_theta_k, args):
    """get_contributors for a matrix held as records (no posterior matrix): the candidates of find_contribs_from_records."""
    return _contributor_table(phylo, obs, haplogroups, props,
                              lambda: find_contribs_from_records(cm, ln_theta_k, wts, args), args)


def read_votes(read_hap_mat):
    """Counter {column: number of rows voting for it}, unweighted (stats.py:39-40),
    with the reference's insertion order so that most_common() breaks ties alike."""
    best, votes = _row_argmax_votes_device(read_hap_mat, None)
    _, order, votes_h = _contributors_on_device(best, votes, votes.numel(), 0)
    counter = collections.Counter()
    for h in order:
        counter[int(h)] = int(votes_h[h])
    return counter


def report_read_votes(haplogroups, read_hap_mat, top_n=10):
    """stats.report_read_votes (stats.py:34-45), same text on stderr."""
    sys.stderr.write("\nTop 10 haplogroups by read probabilities...\n")
    for hap_i, count in read_votes(read_hap_mat).most_common(top_n):
        sys.stderr.write("%s\t%d\n" % (haplogroups[hap_i], count))
    sys.stderr.write("\n")


def update_contribs(contribs, em_results, haps):
    """assemble.update_contribs (assemble.py:211-230): refined proportions by name."""
    props, _ = em_results
    by_hap = {haps[i]: props[i] for i in range(len(haps))}
    for con in contribs:
        con[2] = by_hap[con[1]]
    return contribs


class AssignedReads(collections.abc.Mapping):
    """
    assign_read_indexes' result -- contributor name -> set of row indexes, plus 'unassigned' (assemble.py:284-334) -- held
    as ONE small integer per row: the sets are only formed when someone looks at them (a 10^6-row table of Python
    integers costs 40 ms to build and nothing downstream of the EM needs it before a writer asks).  Behaves like the
    reference's defaultdict(set) for reading: keys are the names that got at least one row (contributors in their
    order, then 'unassigned'), table[name] is a set (empty for a name without rows), dict(table) the reference's dict.
        count(name)   rows of `name` without forming the set
        rows(name)    their indexes as a numpy array (ascending)
    """

    def __init__(self, assigned, names):
        self._assigned = numpy.asarray(assigned)             # ordinal of the contributor, -1 = unassigned
        self._names = list(names)
        counts = numpy.bincount(self._assigned[self._assigned >= 0], minlength=len(self._names)) if self._assigned.size \
            else numpy.zeros(len(self._names), dtype=numpy.int64)
        self._counts = {name: int(counts[i]) for i, name in enumerate(self._names)}
        n_un = int((self._assigned < 0).sum())
        self._keys = [name for name in self._names if self._counts[name] > 0]
        if n_un:
            self._counts["unassigned"] = n_un
            self._keys.append("unassigned")
        self._sets = {}

    def rows(self, name):
        if name == "unassigned" and "unassigned" not in self._names:
            return numpy.flatnonzero(self._assigned < 0)
        if name not in self._names:
            return numpy.zeros(0, dtype=numpy.int64)
        return numpy.flatnonzero(self._assigned == self._names.index(name))

    def count(self, name):
        return self._counts.get(name, 0)

    def __getitem__(self, name):
        got = self._sets.get(name)
        if got is None:
            got = set(self.rows(name).tolist())
            if name in self._keys:
                self._sets[name] = got
        return got

    def __iter__(self):
        return iter(self._keys)

    def __len__(self):
        return len(self._keys)

    def __contains__(self, name):
        return name in self._keys

    def __eq__(self, other):
        try:
            return dict(self) == dict(other)
        except (TypeError, ValueError):
            return NotImplemented

    def __repr__(self):
        return "AssignedReads(%s)" % ", ".join("%s: %d" % (k, self._counts[k]) for k in self._keys)


def assign_read_indexes(contribs, em_results, haps, reads, min_fold):
    """
    assemble.assign_read_indexes (assemble.py:284-334): contributor name -> set
    of row indexes, plus 'unassigned'; a row goes to its best contributor when,
    after dividing out the mixture proportions, it beats the runner-up by
    min_fold.  One gather kernel (mxm_assign_reads) instead of an argsort of
    all H columns per row; the result is an AssignedReads (one integer per row, sets formed on demand).
    """
    return _assign_rows(contribs, em_results, haps, len(reads), min_fold)[0]


def _assign_rows(contribs, em_results, haps, n_rows, min_fold):
    """assign_read_indexes' AssignedReads and the per-row ordinals it was made from, still on the device (None with one
    contributor or fewer: every row is the first's)."""
    props, read_hap_mat = em_results
    names = [hap_n for hap_n, _, _ in contribs]
    if len(contribs) <= 1:
        return AssignedReads(numpy.zeros(n_rows, dtype=numpy.int32), names[:1]), None
    lib = _lib.load()
    dev = require_gpu()
    mat = as_device(read_hap_mat, torch.float64, dev)
    with numpy.errstate(divide="ignore"):
        log_props = numpy.log(numpy.asarray(props, dtype=numpy.float64))
    cols = numpy.array([haps.index(group) for _, group, _ in contribs], dtype=numpy.int32)
    lp_d = torch.from_numpy(log_props).to(dev)
    cols_d = torch.from_numpy(cols).to(dev)
    assigned = torch.empty(n_rows, dtype=torch.int32, device=dev)
    if n_rows:
        _lib.check(lib.mxm_assign_reads(mat.data_ptr(), mat.stride(0), lp_d.data_ptr(), cols_d.data_ptr(),
                                        len(cols), n_rows, mat.shape[1], float(numpy.log(min_fold)),
                                        assigned.data_ptr(), current_stream()), "mxm_assign_reads")
    return AssignedReads(assigned.cpu().numpy(), names), assigned


class ContribReads(collections.abc.Mapping):
    """
    assemble.assign_reads' result -- contributor name -> that contributor's alignments (assemble.py:233-264) -- held as
    ONE int32 label per alignment on the device: label k < n_contribs is contribs[k], label n_contribs 'unassigned'
    (two contributors or more), -1 an alignment whose fragment is in no row (it is in no table, as in the reference,
    where its read id is in no row's list).
        labels        int32 device tensor [n_aln]; names: the label -> name list
        joined        int32 device tensor [n_aln]: the extension round in which the alignment entered its list (0 =
                      assign_reads; assemble.extend_assemblies writes it) -- the order of a list is (joined, index)
        relabel(labels, joined=None)   take new labels (assemble's extension): counts and host copies are refreshed
        len(cr[name]) that contributor's alignment count (the "Reads" column of report_contributors)
        rows(name)    its alignment indexes (ascending: the file order the reference's lists keep), numpy int64
        as_dict(alns) the reference's dict: name -> [alns[i] for i in rows(name)] (indexes when alns is None)
    Behaves like the reference's defaultdict(list): the keys are the names that got alignments (in the order the
    AssignedReads lists them), and looking up another name adds it as a key with no alignments -- bin/mixemt's
    report_contributors does that for every contributor before write_statistics iterates the keys.
    """

    def __init__(self, cols, labels, names, keys, dcols=None, frag=None):
        self.cols = cols                                     # alignments.AlignmentColumns the labels index
        self.names = list(names)
        self._keys = list(keys)
        self._dcols = dcols
        self._frag = frag                                    # cols.frag on the device (made on demand)
        self.rounds = 0                                      # extension rounds these labels have been through
        self.relabel(labels, torch.zeros(labels.numel(), dtype=torch.int32, device=labels.device))

    def relabel(self, labels, joined=None):
        """Take new labels (and, when given, the rounds the alignments joined their lists in); the names and the keys
        stay what they are."""
        self.labels = labels
        if joined is not None:
            self.joined = joined
        n_labels = len(self.names)
        lab = labels[labels >= 0]
        self._counts = torch.bincount(lab.to(torch.int64), minlength=n_labels).cpu().numpy() if lab.numel() \
            else numpy.zeros(n_labels, dtype=numpy.int64)
        self._host = None

    def device_frag(self):
        """cols.frag (the alignments' fragment = query name) on the device, made once."""
        if self._frag is None:
            self._frag = torch.from_numpy(numpy.ascontiguousarray(self.cols.frag, dtype=numpy.int64)).to(self.labels.device)
        return self._frag

    def device_columns(self):
        """The alignments uploaded for the labelled pileup (observe.DeviceColumns), made once."""
        if self._dcols is None:
            from .observe import DeviceColumns
            self._dcols = DeviceColumns(self.cols, self.labels.device)
        return self._dcols

    def label_of(self, name):
        """The label of `name`, or None for a name without one (a key looked up that is no contributor)."""
        try:
            return self.names.index(name)
        except ValueError:
            return None

    def count(self, name):
        k = self.label_of(name)
        return 0 if k is None else int(self._counts[k])

    def rows(self, name):
        k = self.label_of(name)
        if k is None or not self._counts[k]:
            return numpy.zeros(0, dtype=numpy.int64)
        if self._host is None:
            self._host = self.labels.cpu().numpy()
        return numpy.flatnonzero(self._host == k)

    def as_dict(self, alns=None):
        if alns is None:
            return {name: self.rows(name).tolist() for name in self._keys}
        return {name: [alns[i] for i in self.rows(name)] for name in self._keys}

    def __getitem__(self, name):
        if name not in self._keys:
            self._keys.append(name)                          # (defaultdict(list): the lookup makes the key)
        return self.rows(name)

    def __iter__(self):
        return iter(list(self._keys))

    def __len__(self):
        return len(self._keys)

    def __contains__(self, name):
        return name in self._keys

    def __repr__(self):
        return "ContribReads(%s)" % ", ".join("%s: %d" % (k, self.count(k)) for k in self._keys)


def _row_groups(cols, reads):
    """(ptr, frag) of the rows' fragments: a ReadIdGroups' own arrays, or the reference's list of read-id lists mapped
    to fragment indexes of cols.names."""
    if hasattr(reads, "ptr") and hasattr(reads, "frag"):
        return numpy.asarray(reads.ptr, dtype=numpy.int64), numpy.asarray(reads.frag, dtype=numpy.int64)
    index = {name: f for f, name in enumerate(cols.names)}
    lens = [len(ids) for ids in reads]
    ptr = numpy.zeros(len(lens) + 1, dtype=numpy.int64)
    numpy.cumsum(lens, out=ptr[1:])
    frag = numpy.array([index[name] for ids in reads for name in ids], dtype=numpy.int64)
    return ptr, frag


def alignment_labels(frag, ptr, group_frag, row_label, n_frag, no_row=-1):
    """
    One int32 label per alignment (device): row_label[row of the alignment's fragment], or `no_row` when its fragment is
    in no row.  frag: the alignments' fragment indexes; ptr / group_frag: the rows' fragments (ReadIdGroups); row_label:
    int32 per row.  All device tensors (frag / group_frag int64, ptr int64).
    """
    dev = row_label.device
    frag_label = torch.full((max(int(n_frag), 1),), int(no_row), dtype=torch.int32, device=dev)
    if group_frag.numel():
        frag_label[group_frag] = torch.repeat_interleave(row_label, ptr[1:] - ptr[:-1],
                                                         output_size=int(group_frag.numel()))
    return frag_label[frag].contiguous() if frag.numel() else torch.zeros(0, dtype=torch.int32, device=dev)


def assign_reads(cols, contribs, em_results, haps, reads, args, dcols=None):
    """
    assemble.assign_reads (assemble.py:233-264) over alignments held as columns (alignments.AlignmentColumns; the
    reference re-reads the BAM file and matches query names): assign_read_indexes' rows, then every alignment of a
    row's fragments goes to that row's contributor (or 'unassigned').  reads: the rows' fragments (the encoder's
    ReadIdGroups, or the reference's list of read-id lists).  Returns a ContribReads, one label per alignment, made on
    the device.  dcols: the columns already uploaded (observe.DeviceColumns), reused by write_statistics.
    """
    dev = require_gpu()
    table, assigned = _assign_rows(contribs, em_results, haps, len(reads), args.min_fold)
    names = [hap_n for hap_n, _, _ in contribs]
    if len(contribs) > 1:
        names.append("unassigned")
        row_label = torch.where(assigned >= 0, assigned, torch.full_like(assigned, len(contribs)))
    else:
        row_label = torch.zeros(len(reads), dtype=torch.int32, device=dev)
    ptr, group_frag = _row_groups(cols, reads)
    n_frag = max(len(cols.names), int(cols.frag.max()) + 1 if len(cols) else 0)
    frag_d = torch.from_numpy(cols.frag).to(dev)
    labels = alignment_labels(frag_d, torch.from_numpy(ptr).to(dev), torch.from_numpy(group_frag).to(dev), row_label,
                              n_frag)
    return ContribReads(cols, labels, names, list(table), dcols, frag_d)
