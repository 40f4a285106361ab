"""generate.py's outputs against a recorded result: tests/golden/generate_bits.json holds, for one run per mode and sampling strategy
(make_golden.py: GENERATE_RUNS), SHA-256 digests of every array of every .npz (dtype, shape and raw bytes), of every .png, of the text
of every .json and of the printed line, as generate.main wrote them at the commit the file names - before the CLI became a table of
modes.  Equality of digests is the only tolerance; a digest that did not repeat within one process at that commit is named in
"not_reproducible" and absent.

Shapes: -b 8 with 5 or 20 images of 64x64 crosses a chunk edge and leaves a ragged last chunk; projections run 3 steps.  The
checkpoints are gpu_util.make_checkpoints'; runs a and c are made once, the other runs read their images.npz."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import DRAW_CAP, GENERATE_RUNS, generate_run, generate_workdir  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_bits.json")) as f:
        rec = json.load(f)
    assert rec["commit"], "the fixture names the commit it was recorded from"
    assert set(rec["runs"]) | set(rec["left_out"]) == set(GENERATE_RUNS) and set(rec["left_out"]) <= {"h"}
    return rec


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("generate_bits")
    return d, generate_workdir(d)


@pytest.mark.parametrize("name", list(GENERATE_RUNS))
def test_generate_bits(golden, workdir, name):
    d, made = workdir
    if name in golden["left_out"]:                     # rejection sampling ran into its draw cap at the recorded commit: it still does
        from hipgan._lib import JckError
        assert DRAW_CAP in golden["left_out"][name]
        with pytest.raises(JckError, match="cap 50"):
            generate_run(d, name)
        return
    want = golden["runs"][name]
    got = made.get(name) or generate_run(d, name)
    left_out = {k for k in got if f"{name}.{k}" in golden["not_reproducible"]}
    assert want and set(want) == set(got) - left_out
    assert {k: got[k] for k in want} == want
