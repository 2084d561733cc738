"""What the two tiers of the cone-build tests share (tests/test_build_emul.py, tests/test_gpu_build.py): the cases and
their restated reductions, computed once, and the comparison of a decoded store / lite store with them.
TEST INFRASTRUCTURE."""

import build_cases as BC
import build_ref as BR
import limit_cones as LC

ST_TOO_LARGE = 2

FULL_LDS = 160 * 1024
SEEDS = (0, 17)          # round robin, one shuffled schedule
FAMILIES = {"A": BC.family_a, "B": BC.family_b, "C": BC.family_c, "D": BC.family_d}
_cases, _refs = {}, {}


def cases_of(fam):
    if fam not in _cases:
        _cases[fam] = FAMILIES[fam]()
    return _cases[fam]


def refs_of(case):
    """the restated reduction of every instance of a case: computed once, shared by every route"""
    if case["name"] not in _refs:
        _refs[case["name"]] = [BR.reduce_instance(a) for a in case["ctrs"]]
    return _refs[case["name"]]


def nnz_cap(ctrs):
    return max(64, int((ctrs != 0).reshape(len(ctrs), -1).sum(1).max(initial=0)))


def check_store(case, arrs, route):
    for b, ref in enumerate(refs_of(case)):
        dec = BR.decode_store(arrs, b)
        if case["family"] == "C":
            ok, why = BR.is_valid_reduction(case["ctrs"][b], dec, ref)
            assert ok, (route, case["name"], b, why)
            assert BR.no_false_pairs(case["ctrs"][b], dec), (route, case["name"], b)
        else:
            BR.record(route, BR.assert_same(dec, ref, (route, case["name"], b)))


def lite_must_pack(ref, ctrs_b, m, d):
    """the pack half must take this instance: the lite form takes the cone and the instance is within what step_limits
    sizes the arena for (non-zeros within the cap, reduced non-zeros within 6/10 of it, <= 64 general rows)"""
    cap = min(max(4 * (m + d) + 128, 64), max(m * d, 64))
    return (BR.lite_takes(ref, d, LC.scratch_fits) and int((ctrs_b != 0).sum()) <= cap
            and int((ref["M"] != 0).sum()) <= cap * 6 // 10 and sum(t == "general" for t in ref["tags"]) <= 64)


def check_lite(case, arrs, status, route, must=None):
    """a lite store against the restatement: state 1 exactly for the cones the lite form takes (from a packed store), or
    -- on the pack halves, whose arena may also refuse -- never 1 for a cone it does not take and always 1 where `must`"""
    ctrs = case["ctrs"]
    d = ctrs.shape[2]
    for b, ref in enumerate(refs_of(case)):
        dec = BR.decode_lite(arrs, b, d)
        takes = BR.lite_takes(ref, d, LC.scratch_fits) if case["family"] != "C" else None
        assert (status[b] == 0) == (dec["state"] == 1) and status[b] in (0, ST_TOO_LARGE), (route, case["name"], b, status[b])
        if case["family"] == "C":
            if dec["state"] == 1:
                ok, why = BR.is_valid_reduction(ctrs[b], dec, ref)
                assert ok and BR.no_false_pairs(ctrs[b], dec), (route, case["name"], b, why)
            continue
        if must is None:
            assert (dec["state"] == 1) == takes, (route, case["name"], b, dec["state"], takes)
        else:
            assert dec["state"] != 1 or takes, (route, case["name"], b)
            assert dec["state"] == 1 or not must[b], (route, case["name"], b, "refused a cone the pack half must take")
        if dec["state"] == 1:
            BR.record(route, BR.assert_same(dec, ref, (route, case["name"], b)))
