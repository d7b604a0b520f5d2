"""
Every entry of the C ABI that takes a `void *stream` (and mxm_preload, which takes none but loads the code object onto
the device) is held to the stream contract by tests/test_gpu_stream_contract.py in exactly one class, or is excused:

  A  only enqueues, capturable        gate pending at return, host time under half the delay, the graph run passes
  B  only enqueues, no capture        uploads host arrays or takes stream-ordered memory of its own
  C  waits                            and its header says so: the sentence is quoted below and looked up in the header
  excused                             the mxm_diag_* measurement hooks outside the boundary

A new stream-taking entry in one of the headers fails this test until it is classified and has a case.  No GPU.
"""
import os
import re

from conftest import ROOT
from test_guarded_complete import HEADERS, declared_entries

import _stream_cases as sc

DIAG = "mxm_diag_*: measurement hooks outside the boundary (include/mixemt_hip_tuning.h)"
EXCUSED = {"mxm_diag_stream_read": DIAG, "mxm_diag_stream_coded": DIAG, "mxm_diag_stream_quads": DIAG}

LOOP = "Blocks the calling thread"
# entry -> (header, the sentence of its paragraph that says that it waits)
WAITS = {
    "mxm_preload": ("mixemt_hip.h", "returns when it is loaded (blocking)"),
    "mxm_em_loop": ("mixemt_hip.h", LOOP + " (stream sync per chunk)"),
    "mxm_em_loop_f32": ("mixemt_hip.h", "mxm_em_loop_f32 blocks the calling thread as mxm_em_loop does"),
    "mxm_em_loop_coded": ("mixemt_hip.h", "mxm_em_loop_coded blocks the calling thread as mxm_em_loop does"),
    "mxm_em_loop_samples": ("mixemt_hip.h", "mxm_em_loop_samples blocks the calling thread; state_host[S] receives the final states"),
    "mxm_observe_bases": ("mixemt_hip.h", "HOST, blocking (stream-ordered scratch of its own; returns once the stream has finished the call's work)"),
    "mxm_observe_bases_labelled": ("mixemt_hip.h", "HOST, blocking, as mxm_observe_bases"),
    "mxm_first_observed": ("mixemt_hip.h", "HOST, blocking (scratch of n_labels * ref_len * 64 bytes"),
    "mxm_extend_assign": ("mixemt_hip.h", "HOST, blocking. Returns 0, -1 (a fragment index outside [0, n_frag))"),
    "mxm_em_loop_samples_narrow": ("mixemt_hip_samples_finish.h", "mxm_em_loop_samples_narrow blocks the calling thread (one read-back of the states per launch); state_host[S] receives the final states"),
}


def header_text(name):
    """The header with its comment decoration gone and its white space collapsed: a sentence may span lines."""
    with open(os.path.join(ROOT, "include", name)) as fin:
        text = fin.read()
    text = re.sub(r"^\s*/?\*+/?", " ", text, flags=re.M)
    return re.sub(r"\s+", " ", text)


def stream_entries():
    """The declared entries with a `void *stream` parameter."""
    names = set()
    for header in HEADERS:
        with open(os.path.join(ROOT, "include", header)) as fin:
            text = fin.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
        for decl in text.split(";"):
            found = re.search(r"\b(mxm_\w+)\s*\((.*)\)", decl, flags=re.S)
            if found and "typedef" not in decl.split(found.group(1))[0] and re.search(r"\bvoid\s*\*\s*stream\b", found.group(2)):
                names.add(found.group(1))
    return names


def test_the_parser_finds_the_51_stream_taking_entries():
    names = stream_entries()
    assert names <= declared_entries()
    assert len(names) == 51, sorted(names)
    for known in ("mxm_em_iter", "mxm_check_variants_samples", "mxm_votes_samples", "mxm_exchange_reduce", "mxm_diag_stream_read",
                  "mxm_fold_logaddexp", "mxm_extend_assign"):
        assert known in names, known
    for no_stream in ("mxm_preload", "mxm_samples_plan", "mxm_aln_encode", "mxm_exchange_create", "mxm_diag_fused_stamps"):
        assert no_stream not in names, no_stream


def test_every_stream_taking_entry_is_in_exactly_one_class_or_excused():
    names = stream_entries() | {"mxm_preload"}
    classes = {k: set(sc.entries_of(k)) for k in "ABC"}
    for a, b in (("A", "B"), ("A", "C"), ("B", "C")):
        assert not (classes[a] & classes[b]), "in two classes: %r" % sorted(classes[a] & classes[b])
    classified = classes["A"] | classes["B"] | classes["C"]
    assert not (classified & set(EXCUSED)), sorted(classified & set(EXCUSED))
    assert not (set(EXCUSED) - names), "excused names that are no stream-taking entry: %r" % sorted(set(EXCUSED) - names)
    assert all(name.startswith("mxm_diag_") and EXCUSED[name] for name in EXCUSED)
    missing = sorted(names - classified - set(EXCUSED))
    assert not missing, "stream-taking entries without a case in tests/_stream_cases.py: %r" % missing
    assert not (classified - names), "cases of names that are no stream-taking entry: %r" % sorted(classified - names)
    assert len(classified) + len(EXCUSED) == 52


def test_every_case_is_in_its_entrys_class_and_the_ids_are_unique():
    assert len(set(sc.ids())) == len(sc.TABLE)
    for entry, route, klass, _ in sc.TABLE:
        assert klass in "ABC" and route, (entry, route, klass)
    for entry in sc.HOST_ARRAY_ENTRIES:
        assert entry in sc.entries_of(), entry


def test_every_waiting_entry_quotes_the_header_sentence_that_says_so():
    assert set(WAITS) == set(sc.entries_of("C")), (sorted(set(WAITS) ^ set(sc.entries_of("C"))))
    texts = {}
    for entry, (header, sentence) in sorted(WAITS.items()):
        text = texts.setdefault(header, header_text(header))
        assert re.sub(r"\s+", " ", sentence) in text, "%s: %s does not say %r" % (entry, header, sentence)


BLOCKING = re.compile(r"\bBlocks\b|\bblocks the calling\b|\bblocking\b|may wait for")


def blocking_claims(header):
    """[(sentence, entries it names, entries declared behind its comment)] for every sentence of a comment of the header
    that speaks of the HOST waiting (a kernel that spins on a flag "waits" too: that is not meant)."""
    with open(os.path.join(ROOT, "include", header)) as fin:
        text = fin.read()
    every = declared_entries()
    out = []
    parts = re.split(r"(/\*.*?\*/)", text, flags=re.S)                   # code, comment, code, comment, ...
    for at in range(1, len(parts), 2):
        behind = set()
        for code in parts[at + 1::2]:                                     # the declarations up to the next block comment
            behind |= set(re.findall(r"\b(mxm_\w+)\s*\(", code))
            if code.strip().endswith(";") and behind:
                break
        comment = re.sub(r"\s+", " ", re.sub(r"^\s*/?\*+/?", " ", parts[at], flags=re.M))
        for sentence in re.split(r"(?<=[.;])\s+", comment):
            if BLOCKING.search(sentence):
                named = {n for n in every if re.search(r"\b%s\b" % re.escape(n), sentence)}
                out.append((sentence.strip(), named, behind & every))
    return out


def test_no_paragraph_of_an_entry_that_only_enqueues_claims_to_block():
    """The other half of "the headers and the table agree": a sentence that says the host blocks or may wait names an entry
    outside classes A and B and none inside them; where it names nobody, every entry declared behind its comment is outside
    them."""
    enqueues = set(sc.entries_of("A")) | set(sc.entries_of("B"))
    seen = 0
    for header in HEADERS:
        for sentence, named, behind in blocking_claims(header):
            seen += 1
            assert not (named & enqueues), "%s: %r says that %r block(s)" % (header, sentence, sorted(named & enqueues))
            subject = named if named else behind
            assert subject and not (subject & enqueues), "%s: %r stands over %r" % (header, sentence, sorted(subject & enqueues))
    assert seen >= len(WAITS) - 1                      # (every waiting entry has its sentence; two loops share one)


def test_the_conventions_name_the_exceptions():
    text = header_text("mixemt_hip.h")
    assert "every call only enqueues work on it unless stated otherwise" in text
    assert "hipMallocAsync" in text and "hipGraph-capturable" in text
