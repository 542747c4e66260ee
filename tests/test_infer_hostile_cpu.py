"""The planted cases of tests/infer_cases.py on the host: no GPU, nothing loaded into Python.
  Agreement: for every case and every pass - Viterbi decode, smoothing, E-step / M-step / fit, pairwise read-outs, path sampler -
    the stand-alone program over the pass's restatement header (hammlet_amd/csrc/hml_*_ref.h), plain and under the address and
    undefined-behaviour sanitizers, equals the Python restatement word for word, through the checks of the passes' own CPU tests.
  Coverage: the table is not vacuous - every case holds the mechanism it is in the table for, and every flag of
    infer_cases.FLAGS is held by some case; decided from the Python restatements alone."""
import numpy as np
import pytest

from tests import em_util as eu
from tests import infer_cases as ic
from tests import pairs_util as pz
from tests import posterior_util as pu
from tests import sample_util as su
from tests import viterbi_util as vu
from tests.test_em_cpu import check_case as check_em
from tests.test_pairs_cpu import check_case as check_pairs
from tests.test_posterior_cpu import check as check_posterior
from tests.test_sample_cpu import check_case as check_sample
from tests.test_viterbi_cpu import check as check_viterbi

NAMES = sorted(ic.CASES)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("infer_hostile")
    out = {}
    for name, util in (("viterbi", vu), ("posterior", pu), ("em", eu), ("pairs", pz), ("sample", su)):
        sub = d / name
        sub.mkdir()
        out[name] = util.build_programs(sub)
    out["sample"] = (out["sample"], str(d / "sample"))
    return out


def restated(case):
    """the results ic.flags() reads, from the Python restatements alone"""
    with np.errstate(all="ignore"):
        e, m = pu.tables(case)
        s = pu.smooth(case, e, m)
        emit, trans, init = vu.tables(case)
        path, score, _, _ = vu.decode(emit, trans, init)
        n = eu.estep(case)
        t = pz.terms(case)
        draws = su.restate(case, 0, 8, 7)
        reasons = [eu.fit(case, 3, 0.0, prior_on, eu.FLAT)[3] for prior_on in (False, True)]
    return dict(degenerate=s["degenerate"], loglik=s["loglik"], e=np.array(e, np.float32), emit=emit, score=score, score_plain=vu.path_score(path, emit, trans, init),
                xi_degenerate=n["xi_degenerate"], pair_degenerate=t["pair_degenerate"], sample_degenerate=draws["sample_degenerate"], reasons=reasons,
                occ=n["occ"], sx=n["sx"], sxx=n["sxx"])


@pytest.fixture(scope="module")
def held():
    """name -> the flags the case holds"""
    return {name: ic.flags(c, restated(c)) for name, c in ((name, ic.case(name)) for name in NAMES)}


def test_the_table_holds_what_the_issue_lists():
    cases = {name: ic.case(name) for name in NAMES}
    assert {c["K"] for c in cases.values()} >= {2, 5, 20}
    assert any((c["D"], c["P"]) == (2, 2) for c in cases.values())
    lens = np.diff(cases["sticky_5000"]["starts"].astype(np.int64))
    assert lens.tolist() == [5000] * 10
    assert cases["var_denormal"]["mean_var"][1] == np.float32(2.0 ** -149) > 0
    assert all(len(c["starts"]) - 1 >= 65 for name, c in cases.items() if "clamped_and_wrapped" in ic.EXPECT[name])


@pytest.mark.parametrize("name", NAMES)
def test_every_case_holds_its_mechanism(held, name):
    assert ic.EXPECT[name] <= held[name], (name, sorted(ic.EXPECT[name] - held[name]))


def test_every_mechanism_is_held_by_some_case(held):
    named = set().union(*ic.EXPECT.values())
    assert named == set(ic.FLAGS), sorted(set(ic.FLAGS) - named)
    # the division branch of the inner product on each of its four grounds, and the common branch
    for flag in ("ip_close", "ip_tiny", "ip_huge", "ip_not_finite", "ip_common"):
        assert any(flag in f for f in held.values()), flag


@pytest.mark.parametrize("name", NAMES)
def test_programs_equal_the_python_restatements(programs, name):
    case = ic.case(name)
    with np.errstate(all="ignore"):
        check_viterbi(programs["viterbi"], case, name)
        check_posterior(programs["posterior"], case, name)
        check_em(programs["em"], case, name)
        check_pairs(programs["pairs"], case, name)
        degenerate = bool({"partly_degenerate", "all_degenerate"} & ic.EXPECT[name])
        if "clamped_and_wrapped" not in ic.EXPECT[name]:
            check_sample(programs["sample"], case, name, count=8, seed=7, degenerate=degenerate)
        else:                                   # (a wrapped score is not bounded by the decode's wrapped score: the words alone)
            exes, d = programs["sample"]
            start, end = pz.edge_regions(case["starts"], np.random.default_rng(11), n_random=3)
            want = su.restate(case, 0, 8, 7, start, end, 3)
            for kind, exe in exes.items():
                got = su.run_program(exe, case, 0, 8, 7, start, end, 3, paths_file=d + "/paths_" + kind)
                assert np.array_equal(got["alpha"], want["alpha"]) and np.array_equal(got["paths"], want["paths"]), (name, kind)
                su.same(got, want, su.COUNT_KEYS + su.REGION_KEYS + ("viterbi_score",), (name, kind))
