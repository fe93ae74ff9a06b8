"""Every output of the profiled-fit kernels `==` what the commit before the shared per-bin helpers and launch layer
gave (csrc/profile_device.hpp: `pf_finite`, `pf_phi`, `pf_prior`, `pf_bound_set`; csrc/profile_kernel.hpp: `pf_check`,
`pf_args_*`, `pf_plan_split`, `pf_run_any`; kernels.py: `_profiled_full`, `_profiled_best`): the six matrix entry
points (`kernels.profiled_metric_matrix` and `_best`, without and with bounds, and their `_wide` forms),
`profiled_hesse` and `posterior_sample`, for the four kinds.

The expectation is tests/golden/profile_parent.npz, recorded once on an MI355X from a build of that commit by
scripts/dev/record_profile_parent.py with the toolchain these tests run under.  It holds no input: the inputs are the
seeded families of tests/profile_cases.py, profile_bounded_cases.py, profile_wide_cases.py, hesse_cases.py and
posterior_cases.py, named by the case list below, which the fixture repeats (`cases`) together with the seeds that are
this module's own (`seeds`).  Per group of calls the int32 outputs and the float64 outputs of at most STORED doubles
are kept in full (doubles as their int64 words), longer ones as the SHA-256 of their bytes.

Shapes (T, K, B, J).  Narrow: J of {1, 8}, B of {1, 16, 17} (both sides of the 16-bin chunk), T of {1, 65} (a strip
with a dead-lane tail), K = 3.  Wide: J of {1, 8, 9, 32}, B of {1, 64, 65}, T of {1, 2}, K = 3.  One reduced case per
form with K = 1030 > PF_MAX_SPLIT templates: `k_chunk` = 2, so the join runs over ranges of more than one template.
Every shape runs without bounds (the unbounded entry points), with a box that binds, with one coordinate pinned and
with one template's box bad.  The status families of the case modules and a `max_iter = 0` call bring every flag.
"""
import hashlib
import json

import numpy as np
import pytest

from tests import hesse_cases as hc
from tests import posterior_cases as po
from tests import profile_bounded_cases as bc
from tests import profile_cases as pc
from tests import profile_wide_cases as wc
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = "profile_parent.npz"
STORED = 64                     # doubles of an output kept as an array; a longer one is kept as a digest
FAMILY = "poisson"              # unit priors on every parameter: J > B is fitted
FORMS = ("narrow", "wide")
BOUNDS = ("none", "binds", "pinned", "bad")
SHAPES = {
    "narrow": tuple((T, 3, B, J) for J in (1, 8) for B in (1, 16, 17) for T in (1, 65)),
    "wide": tuple((T, 3, B, J) for J in (1, 8, 9, 32) for B in (1, 64, 65) for T in (1, 2)),
}
SPLIT_SHAPE = {"narrow": (2, 1030, 3, 2), "wide": (2, 1030, 3, 9)}
SEEDS = dict(offset=20261021, posterior=po.SEED, posterior_stream=3, posterior_chain0=11)
HESSE_SHAPE = (65, 3, 17, 8)
POSTERIOR_CASES = po.GPU_CASES[:5]           # the four kinds, J of {1, 3, 8}, every form of the bounds
HELD = hc.HELD
FLAGS = dict(NOT_CONVERGED=pc.NOT_CONVERGED, BOUNDARY=pc.BOUNDARY, NOT_POSDEF=pc.NOT_POSDEF,
             START_OUTSIDE=pc.START_OUTSIDE, BAD_BOUNDS=bc.BAD_BOUNDS, HELD=HELD)

assert max(s[3] for s in SHAPES["narrow"]) == pc.MAX_PARAMS and max(s[3] for s in SHAPES["wide"]) == wc.MAX_PARAMS


def shape_id(shape):
    return "T%d-K%d-B%d-J%d" % shape


def bounds_of(name, K, J):
    """(lower, upper) as the caller passes them: None, [J] or [K, J]"""
    if name == "none":
        return None, None
    if name == "binds":
        return bc.box("narrow", K, J)                      # [K, J] on both sides
    if name == "pinned":
        lo, hi = (b.copy() for b in bc.box("wide", K, J))  # [J], shared
        lo[0] = hi[0] = 0.01
        return lo, hi
    if name == "bad":
        lo, hi = (b.copy() for b in bc.box("narrow", K, J))
        lo[K // 2, J - 1], hi[K // 2, J - 1] = 0.2, 0.1
        return lo, hi
    raise KeyError(name)


def offset_of(K):
    return np.random.RandomState(SEEDS["offset"]).randn(K)


def case_list():
    """the names of every recorded call, in the order they run"""
    out = []
    for form in FORMS:
        for kind in pc.KINDS:
            for shape in SHAPES[form]:
                out += ["%s/%s/%s/%s" % (form, kind, shape_id(shape), b) for b in BOUNDS]
            out += ["%s/%s/%s/%s" % (form, kind, shape_id(SPLIT_SHAPE[form]), b) for b in ("none", "binds")]
        out += ["%s/status/%s" % (form, n) for n in pc.STATUS_FAMILIES + ("maxiter0",)]
        out += ["%s/status-box/%s" % (form, n) for n in bc.STATUS_FAMILIES]
    out += ["hesse/%s/%s" % (kind, b) for kind in pc.KINDS for b in BOUNDS]
    out += ["posterior/%s" % po.gpu_case_id(q) for q in POSTERIOR_CASES]
    return out


# ----------------------------------------------------------------------------------------------------- the calls
def _dev(K, a, dtype=np.float64):
    import torch

    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(K.device())


def _host(out, prefix):
    return {prefix + "/" + k: v.cpu().numpy() for k, v in out.items() if v is not None}


def matrix_calls(K, form, name, kind, f, lower, upper, k0, max_iter=pc.MAX_ITER, reduced_only=False):
    """{name/full/..., name/best/...}: the full and the reduced output of one case"""
    full = K.profiled_metric_matrix_wide if form == "wide" else K.profiled_metric_matrix
    best = K.profiled_metric_matrix_best_wide if form == "wide" else K.profiled_metric_matrix_best
    args = [_dev(K, f[n]) for n in ("D", "E", "R", "S2", "ips", "c")]
    box = dict(lower=_dev(K, lower), upper=_dev(K, upper))
    out = {}
    if not reduced_only:
        out.update(_host(full(kind, *args, max_iter=max_iter, **box), name + "/full"))
    out.update(_host(best(kind, *args, _dev(K, offset_of(f["E"].shape[0])), k0, max_iter=max_iter, **box),
                     name + "/best"))
    return out


def run_matrix(K, form, kind):
    out = {}
    for shape in SHAPES[form]:
        f = pc.family(FAMILY, *shape)
        for b in BOUNDS:
            lower, upper = bounds_of(b, shape[1], shape[3])
            out.update(matrix_calls(K, form, "%s/%s/%s/%s" % (form, kind, shape_id(shape), b), kind, f, lower, upper, 1))
    shape = SPLIT_SHAPE[form]
    f = pc.family(FAMILY, *shape)
    for b in ("none", "binds"):
        lower, upper = bounds_of(b, shape[1], shape[3])
        out.update(matrix_calls(K, form, "%s/%s/%s/%s" % (form, kind, shape_id(shape), b), kind, f, lower, upper,
                                shape[1] // 2, reduced_only=True))
    return out


def run_status(K, form):
    out = {}
    for n in pc.STATUS_FAMILIES + ("maxiter0",):
        f = dict(pc.family("far", 65, 1, 3, 1), kind="llh", max_iter=0) if n == "maxiter0" else pc.status_family(n)
        out.update(matrix_calls(K, form, "%s/status/%s" % (form, n), f["kind"], f, None, None, 0, f["max_iter"]))
    for n in bc.STATUS_FAMILIES:
        f = bc.status_family(n)
        out.update(matrix_calls(K, form, "%s/status-box/%s" % (form, n), f["kind"], f, f["lower"], f["upper"],
                                min(1, f["E"].shape[0] - 1), f["max_iter"]))
    return out


def run_hesse(K, kind):
    """the fitted points of hesse_cases (the numpy restatement's, without and inside the narrow box), every trial at
    its own template and all at template 1"""
    out = {}
    T, Kn, _, J = HESSE_SHAPE
    for b in BOUNDS:
        f, ks, eta, _, _ = hc.fitted(FAMILY, kind, *HESSE_SHAPE, box="narrow" if b == "binds" else None)
        lower, upper = bounds_of(b, Kn, J)
        args = [_dev(K, f[n]) for n in ("S2", "ips", "c")] + [_dev(K, lower), _dev(K, upper)]
        for tag, k in (("own", _dev(K, ks, np.int32)), ("one", 1)):
            got = K.profiled_hesse(kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["R"]), _dev(K, eta), k, *args)
            out.update(_host(got, "hesse/%s/%s/%s" % (kind, b, tag)))
    return out


def run_posterior(K, q):
    kind, P, B, J, W, bounds, n_steps, first = q
    f = po.case(kind, P, B, J, W, bounds)
    ids = np.arange(P) + SEEDS["posterior_chain0"]
    got = K.posterior_sample(kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["R"]), _dev(K, f["x0"]), n_steps,
                             SEEDS["posterior"], t_of=_dev(K, f["t_of"], np.int32), k_of=_dev(K, f["k_of"], np.int32),
                             sigma2=_dev(K, f["S2"]), inv_prior_sigma=_dev(K, f["ips"]), center=_dev(K, f["c"]),
                             lower=_dev(K, f["lo"]), upper=_dev(K, f["hi"]), stream=SEEDS["posterior_stream"],
                             chain_id=_dev(K, ids, np.int64), first_step=first)
    return _host(got, "posterior/%s" % po.gpu_case_id(q))


# --------------------------------------------------------------------------------------------------- the fixture
def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def to_fixture(group, tables):
    """what the fixture keeps of the outputs {key: array} of one group of calls, as four entries: the list of (key,
    shape, what) and, in that order, the int32 outputs joined, the words of the short float64 outputs joined, and the
    digests of the long ones"""
    keys, ints, words, digests = [], [], [], []
    for key, a in tables.items():
        if a.dtype == np.int32:
            what = "i"
            ints.append(a.ravel())
        elif a.size <= STORED:
            what = "f"
            words.append(np.ascontiguousarray(a).view(np.int64).ravel())
        else:
            what = "h"
            digests.append(digest(a))
        assert a.dtype == (np.int32 if what == "i" else np.float64), (key, a.dtype)
        keys.append([key, list(a.shape), what])
    return {group + ":keys": np.array(json.dumps(keys)), group + ":sha256": np.array(json.dumps(digests)),
            group + ":int32": np.concatenate(ints + [np.zeros(0, np.int32)]),
            group + ":words": np.concatenate(words + [np.zeros(0, np.int64)])}


def from_fixture(golden, group):
    """{key: array} of a group: int32 arrays, int64 words of the short doubles, digests of the long ones"""
    out, at = {}, dict(i=0, f=0, h=0)
    src = dict(i=golden[group + ":int32"], f=golden[group + ":words"], h=json.loads(str(golden[group + ":sha256"])))
    for key, shape, what in json.loads(str(golden[group + ":keys"])):
        n = 1 if what == "h" else int(np.prod(shape, dtype=np.int64))
        part = src[what][at[what]:at[what] + n]
        out[key] = part[0] if what == "h" else part.reshape(shape)
        at[what] += n
    return out


def groups():
    """(group, what runs it) in the order of the recorder"""
    out = [("%s/%s" % (form, kind), lambda K, form=form, kind=kind: run_matrix(K, form, kind))
           for form in FORMS for kind in pc.KINDS]
    out += [("%s/status" % form, lambda K, form=form: run_status(K, form)) for form in FORMS]
    out += [("hesse/%s" % kind, lambda K, kind=kind: run_hesse(K, kind)) for kind in pc.KINDS]
    out += [("posterior/%s" % po.gpu_case_id(q), lambda K, q=q: run_posterior(K, q)) for q in POSTERIOR_CASES]
    return out


def fixture_header():
    return {"cases": np.array(json.dumps(case_list())), "seeds": np.array(json.dumps(SEEDS, sort_keys=True))}


@pytest.fixture(scope="module")
def K():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def golden():
    return load_golden(FIXTURE)


def _check(K, golden, group):
    got = to_fixture(group, dict(groups())[group](K))
    want = from_fixture(golden, group)
    assert str(got[group + ":keys"]) == str(golden[group + ":keys"]), "%s: other outputs than the recorded ones" % group
    for key, a in from_fixture(got, group).items():
        assert np.array_equal(a, want[key]), key
    for name, a in got.items():
        assert np.array_equal(a, golden[name]), name
    return len(want)


def _recorded(golden, head, tail):
    """the recorded int32 outputs whose key begins with `head` and ends with `tail`, joined"""
    parts = [a.ravel() for group, _ in groups() if group.startswith(head.split("/")[0])
             for key, a in from_fixture(golden, group).items() if key.startswith(head) and key.endswith(tail)]
    return np.concatenate(parts)


# ----------------------------------------------------------------------------------------------------- the tests
def test_fixture_is_of_these_cases_and_holds_every_flag(golden):
    assert json.loads(str(golden["cases"])) == case_list()
    assert json.loads(str(golden["seeds"])) == json.loads(json.dumps(SEEDS))
    names, seen = set(case_list()), set()
    for group, _ in groups():
        for key in from_fixture(golden, group):
            name = [n for n in names if key.startswith(n + "/")]
            assert len(name) == 1, key
            seen.add(name[0])
    assert seen == names
    solver = ("NOT_CONVERGED", "BOUNDARY", "NOT_POSDEF", "START_OUTSIDE", "BAD_BOUNDS")
    for form in FORMS:
        for output in ("/full/status", "/best/status"):
            flags = _recorded(golden, form + "/", output)
            for name in solver:
                assert (flags & FLAGS[name]).any(), (form, output, name)
            assert not (flags & ~sum(FLAGS[name] for name in solver)).any()
        # out of iterations at max_iter = 0, and given up after the halvings of one step with iterations to spare
        assert (_recorded(golden, form + "/status/maxiter0/", "/full/status") == pc.NOT_CONVERGED).all()
        assert not _recorded(golden, form + "/status/maxiter0/", "/full/n_iter").any()
        st = _recorded(golden, form + "/status/boundary/", "/full/status")
        it = _recorded(golden, form + "/status/boundary/", "/full/n_iter")
        assert ((st & pc.NOT_CONVERGED) != 0)[it < pc.MAX_ITER].any()
    hesse = _recorded(golden, "hesse/", "/status")
    for name in ("HELD", "BAD_BOUNDS"):
        assert (hesse & FLAGS[name]).any(), ("hesse", name)
    assert (hesse == 0).any()


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("form", FORMS)
def test_matrix_entry_points_give_the_parents_bits(K, golden, form, kind):
    n = _check(K, golden, "%s/%s" % (form, kind))
    print("%s %s: %d outputs equal to the recorded ones" % (form, kind, n))


@pytest.mark.parametrize("form", FORMS)
def test_flagged_pairs_give_the_parents_bits(K, golden, form):
    _check(K, golden, "%s/status" % form)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_hesse_gives_the_parents_bits(K, golden, kind):
    _check(K, golden, "hesse/%s" % kind)


@pytest.mark.parametrize("q", POSTERIOR_CASES, ids=po.gpu_case_id)
def test_posterior_gives_the_parents_bits(K, golden, q):
    _check(K, golden, "posterior/%s" % po.gpu_case_id(q))
