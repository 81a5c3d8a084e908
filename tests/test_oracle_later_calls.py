"""The oracle's later liblqr calls (oracle/lqr_oracle.c: the gdouble masks, the _xy entries, the clears, lqr_carver_get_true_energy and
the two plane hooks) pinned, without a GPU, to what the genuine liblqr 0.4.1 recorded under tests/golden/masks/ and tests/golden/energy/.

Every vector of the two manifests is run on the oracle through the drivers the engine's own tests use (mask_cases.run,
energy_cases.run) and compared with assert_same_record: every return value, the orientation after every read-out, both mask planes
and every energy plane at 0 ULP, the pictures byte for byte, and -- what pins the state the calls leave behind -- the image and the
seam map of every resize that follows.  The normalised energy and the picture are energy_cases.normalised / picture of the oracle's
true plane (tests/lqr_ctypes.py, OracleCarver.energy_call).

A vector is left out only by the rule `left_out` states on its spec: the oracle is 8-bit, has no image types and no more than 4
channels, and has no device; the vectors under "findings" are those on which include/lqr_masks.h / lqr_energy.h say the engine (and
with it the oracle's memory-safe restatement) does not follow liblqr.  The test asserts that every other vector ran.
"""
import json
import os

import numpy as np
import pytest

import energy_cases as EC
import lqr_ctypes as L
import mask_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"masks": MC, "energy": EC}
MANIFESTS = {k: json.load(open(os.path.join(ROOT, "tests", "golden", k, "MANIFEST.json"))) for k in FAMILIES}


def left_out(spec):
    """why the oracle cannot run this spec, or None.  (There is no device-memory form in either manifest's op list: the device
    forms are engine extensions the genuine liblqr could not record; an op naming one would be left out here.)"""
    if spec.get("depth", 0) != 0:
        return "a deep depth"
    if spec.get("type") is not None or spec["ch"] > 4 or spec.get("max_ch"):
        return "an image type or more than 4 channels"
    if any("device" in str(op[0]) for op in spec["ops"]):
        return "a device-memory form"
    return None


def vectors(family):
    return [(v["name"], v["spec"]) for v in MANIFESTS[family]["vectors"]]


ELIGIBLE = [(f, name) for f in FAMILIES for name, spec in vectors(f) if left_out(spec) is None]


@pytest.fixture(scope="module")
def orc():
    return L.bind_energy(L.bind_masks(L.oracle_api()))


def reproduce(orc, family, name):
    entry = next(v for v in MANIFESTS[family]["vectors"] if v["name"] == name)
    z = np.load(os.path.join(ROOT, "tests", "golden", family, entry["file"]))
    spec = json.loads(str(z["spec"]))
    assert spec == entry["spec"]
    got = FAMILIES[family].run(orc, L.OracleCarver, spec)
    FAMILIES[family].assert_same_record(got, z, "%s/%s" % (family, name))


@pytest.fixture(scope="module")
def outcomes(orc):
    """(family, name) -> None, or the AssertionError: every vector the rule does not name is run here, once, whichever tests are
    selected and in whatever order"""
    out = {}
    for family, name in ELIGIBLE:
        try:
            reproduce(orc, family, name)
            out[family, name] = None
        except AssertionError as ex:
            out[family, name] = ex
    return out


@pytest.mark.parametrize("family,name", ELIGIBLE, ids=["%s-%s" % e for e in ELIGIBLE])
def test_oracle_reproduces_the_genuine_vector(outcomes, family, name):
    if outcomes[family, name] is not None:
        raise outcomes[family, name]


def test_every_vector_outside_the_rule_ran(outcomes):
    """a condition, not a count: whatever the rule does not name has been run and reproduced"""
    for family in FAMILIES:
        names = [n for n, _ in vectors(family)]
        assert len(names) == len(set(names)) and names
        for name, spec in vectors(family):
            why = left_out(spec)
            assert (why is None) == ((family, name) in outcomes), (family, name, why)
            assert why is not None or outcomes[family, name] is None, (family, name, outcomes[family, name])
        finding_names = {v["name"] for v in MANIFESTS[family]["findings"]}
        assert not finding_names & set(names)               # the findings are a list of their own: none is a vector
    out = sorted((f, n, left_out(s)) for f in FAMILIES for n, s in vectors(f) if left_out(s))
    print("left out by the rule: %s" % out)
    assert {w for _, _, w in out} <= {"a deep depth", "an image type or more than 4 channels", "a device-memory form"}


def test_bind_helpers_bind_the_oracle(orc):
    for name in ("lqr_carver_bias_add_area", "lqr_carver_bias_add", "lqr_carver_rigmask_add_area", "lqr_carver_rigmask_add",
                 "lqr_carver_bias_add_xy", "lqr_carver_rigmask_add_xy", "lqr_carver_bias_clear", "lqr_carver_rigmask_clear",
                 "lqrx_carver_get_bias", "lqrx_carver_get_rigmask", "lqr_carver_get_true_energy"):
        assert getattr(orc, name, None) is not None, name
    for name in L.ORACLE_ABSENT:
        assert not hasattr(orc, name), name
