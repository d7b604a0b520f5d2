"""
Plain numpy / Python restatements for the detection bootstrap (include/mixemt_hip_detect.h; assign.detect_many), shared by
tests/test_detect_host.py and the GPU tests: the candidate rule of mxm_detect_candidates and the host summary of
detect_many.  Written from the header's and the docstring's words, not from the code under test.
"""
import math

LDS = (4, 8, 16, 32, 64)


def candidates(votes, first, n_rows, props, min_reads, ld, state=None):
    """One entry: (ncand, cand, cprop) with cand / cprop lists of length ncand (empty when ncand is -1 or above ld).
    state: None or (done, error)."""
    n_haps = len(votes)
    if any(math.isnan(float(v)) for v in votes):
        return -1, [], []
    if state is not None and (state[1] != 0 or state[0] == 0):
        return -1, [], []
    found = [h for h in range(n_haps) if int(first[h]) < int(n_rows) and float(votes[h]) >= float(min_reads)]
    if any(math.isnan(float(props[h])) for h in found):
        return -1, [], []
    if len(found) > ld:
        return len(found), [], []
    # the reference: the vote table's first-seen order, then the stable sort(reverse=True) by proportion
    table = sorted(found, key=lambda h: int(first[h]))
    contrib_prop = [[h, float(props[h])] for h in table]
    contrib_prop.sort(key=lambda con: con[1], reverse=True)
    return len(found), [con[0] for con in contrib_prop], [con[1] for con in contrib_prop]


FAILED = ("the EM loop did not finish", "poisoned: a NaN vote or proportion, or a loop error", "more than 64 candidates",
          "the variant check left it alone (ncand)", "a candidate index outside the tree")


def summary(cand, ncand, keep, flag, done, contribs, haplogroups):
    """The host summary of one sample, from the words of detect_many's docstring."""
    index = {}
    for i, hap in enumerate(haplogroups):
        index.setdefault(hap, i)
    estimate = {}
    for _, hap, prop in contribs:
        estimate.setdefault(index[hap], prop)
    candidate = dict.fromkeys(estimate, 0)
    kept_count = dict.fromkeys(estimate, 0)
    failed, sizes, order, counts, used, same = {}, {}, [], {}, 0, 0
    for b in range(len(ncand)):
        why = None
        if done[b] == 0:
            why = FAILED[0]
        elif ncand[b] < 0:
            why = FAILED[1]
        elif ncand[b] > 64:
            why = FAILED[2]
        elif flag[b] == 1:
            why = FAILED[3]
        elif flag[b] != 0:
            why = FAILED[4]
        if why:
            failed[why] = failed.get(why, 0) + 1
            continue
        used += 1
        kept = set()
        for i in range(ncand[b]):
            h = int(cand[b][i])
            candidate[h] = candidate.get(h, 0) + 1
            kept_count.setdefault(h, 0)
            if keep is None or keep[b][i]:
                kept_count[h] += 1
                kept.add(h)
        key = tuple(sorted(kept))
        sizes[len(key)] = sizes.get(len(key), 0) + 1
        if key not in counts:
            order.append(key)
            counts[key] = 0
        counts[key] += 1
        same += kept == set(estimate)
    rows = sorted(candidate, key=lambda h: (-kept_count[h], h))
    top = sorted(order, key=lambda key: -counts[key])[:10]
    return {"detection": [[haplogroups[h], candidate[h], kept_count[h], h in estimate, estimate.get(h)] for h in rows],
            "n_used": used, "n_failed": failed, "set_sizes": dict(sorted(sizes.items())), "same_set": same,
            "sets": [([haplogroups[h] for h in key], counts[key]) for key in top]}
