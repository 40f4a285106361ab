"""The plain latent entry points against a recorded result: tests/golden/latent_plain_bits.json holds SHA-256 digests of the raw output
bytes of jck_latent_loss, jck_engine_latent_grad and a 3-step jck_engine_project as the library computed them at the commit the file
names, when the plain calls still had a kernel and a native path of their own.  They are forwarders to the `_ex` path now, so a
comparison of plain with `_ex` compares a path with itself; this file compares both with what the separate implementation gave.
Equality of digests is the only tolerance.  Inputs and recipe: tests/golden/make_golden.py (latent_loss_bits, latent_engine_bits).

Shapes: hw = 64 is below one pass of the loss kernel's 256-thread loop and hw = 4096 is 16 passes; n = 5 of a batch-8 engine leaves a
ragged batch; CGAN adds the label rows."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import LATENT_ENGINES, LATENT_LOSS_CASES, latent_engine_bits, latent_loss_bits  # noqa: E402

pytestmark = pytest.mark.gpu
FORMS = [pytest.param(False, id="plain"), pytest.param(True, id="ex")]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latent_plain_bits.json")) as f:
        rec = json.load(f)
    assert rec["commit"], "the fixture names the commit it was recorded from"
    return rec


@pytest.mark.parametrize("ex", FORMS)
@pytest.mark.parametrize("n,hw,prec", [pytest.param(n, hw, p, id=f"{n}x{hw}-{p}") for n, hw, p in LATENT_LOSS_CASES])
def test_latent_loss_bits(golden, n, hw, prec, ex):
    assert latent_loss_bits(n, hw, prec, ex) == golden["latent_loss"][f"{n}x{hw}-{prec}"]


@pytest.mark.parametrize("ex", FORMS)
@pytest.mark.parametrize("family,prec", [pytest.param(f, p, id=f"{f}-{p}") for f, p in LATENT_ENGINES])
def test_latent_grad_and_project_bits(golden, family, prec, ex):
    assert latent_engine_bits(family, prec, ex) == golden["engine"][f"{family}-{prec}"]
