"""The inference paths against a recorded result: tests/golden/infer_bits.json holds SHA-256 digests of the raw output bytes of
jck_engine_latent_grad_ex / _fm and 3-step jck_engine_project_ex / _fm with a per-pixel weight, a critic and a feature term, of
jck_engine_score and jck_engine_features, and of DcganEngine.latent_grad / critic_grad / project / refine, as the library and the
Python layer computed them at the commit the file names - before the objective, the buffer groups and the chunk loops of these paths
were each written down once.  Equality of digests is the only tolerance.  Inputs and recipe: tests/golden/make_golden.py
(infer_inputs, infer_bits); a digest that did not repeat within one process at that commit is named in "not_reproducible" and absent.

Shapes: n = 5 of a batch-8 64x64 engine leaves a ragged batch; the two families cover both heads, the three precisions both forms of a
D stage; the feature term sits at the first, an inner and the deepest stage, with and without a critic above it."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import INFER_ENGINES, INFER_GROUPS, infer_bits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infer_bits.json")) as f:
        rec = json.load(f)
    assert rec["commit"], "the fixture names the commit it was recorded from"
    return rec


@pytest.mark.parametrize("group", INFER_GROUPS)
@pytest.mark.parametrize("family,prec", [pytest.param(f, p, id=f"{f}-{p}") for f, p in INFER_ENGINES])
def test_infer_bits(golden, family, prec, group):
    want = golden["engine"][f"{family}-{prec}"][group]
    got = infer_bits(family, prec, group)
    left_out = {k for k in got if f"{family}-{prec}.{group}.{k}" in golden["not_reproducible"]}
    assert want and set(want) == set(got) - left_out
    assert {k: got[k] for k in want} == want
