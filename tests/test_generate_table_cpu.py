"""generate.py's table of run modes.

The parser against a recorded result: tests/golden/generate_cli.json holds, for 8758 command lines (make_golden.py: cli_lines - every
0, 1 or 2 of 58 units, and every complete selector with every pair of 22 units, under -m DCGAN and -m CGAN), whether the parser of the
commit the file names refused the line, else a digest of the namespace it returned; the full namespace of the empty and the one-unit
lines, so that a difference can be read.  Equality is the only tolerance and no line is left out.

A mode added here, known to no other code, shows what the table is for: the generic rules hold for it."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import CLI_MODELS, CLI_SELECTORS_B, cli_lines, cli_table  # noqa: E402

BASE = ["--checkpoint", "c.pt", "--out", "o"]


def test_parser_table_is_the_recorded_one():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_cli.json")) as f:
        want = json.load(f)
    assert want["commit"] and len(want["attrs"]) >= 38                           # every attribute the namespace had then
    got = cli_table(want["attrs"])
    assert got["full"] == want["full"]
    for which, lines, accepted in (("A", 3424, 553), ("B", 5334, 987)):
        assert sum(len(want[which][m]) for m in CLI_MODELS) == lines and sum(d != "x" for m in CLI_MODELS for d in want[which][m]) == accepted
        for model in CLI_MODELS:
            differ = [line for line, g, w in zip(cli_lines(which), got[which][model], want[which][model]) if g != w]
            assert len(got[which][model]) == len(want[which][model]) and not differ, (which, model, len(differ), differ[:10])


@pytest.fixture
def echo_mode():
    """a throw-away mode: a selector, one option of its own with a default, a plan that returns its argument"""
    import generate
    m = generate.Mode(name="echo", flag="echo", doc="--echo FILE.npz hands its arguments back (a mode of the test suite).",
                      arguments=(("--echo", dict(metavar="FILE.npz")), ("--echo_gain", dict(type=float))),
                      defaults={"echo_gain": 2.0}, plan=lambda a: a)
    generate.MODES.append(m)
    yield m
    generate.MODES.remove(m)


def test_a_mode_added_to_the_table_obeys_the_generic_rules(echo_mode, capsys):
    import generate
    a = generate.get_arg_parse(BASE + ["--echo", "e.npz"])
    assert a.mode == "echo" and a.echo_gain == 2.0 and generate.mode_of(a) is echo_mode and echo_mode.plan(a) is a
    assert generate.needs_discriminator(a) and a.num == 64 and a.k == 4
    assert generate.get_arg_parse(BASE + ["--echo", "e.npz", "--echo_gain", "3", "--bn", "batch", "--k", "2"]).echo_gain == 3.0
    a = generate.get_arg_parse(BASE)
    assert a.mode == "sample" and a.echo is None and a.echo_gain is None                 # its default is applied only with it
    selectors = [s for s in CLI_SELECTORS_B if s.split()[0] in ("--project", "--score_images", "--features", "--probe", "--inpaint", "--anomaly")]
    assert len(selectors) == len(generate.MODES) - 2
    for s in selectors:                                                                  # refused together with each existing selector
        with pytest.raises(SystemExit):
            generate.get_arg_parse(BASE + ["--echo", "e.npz"] + s.split())
        err = capsys.readouterr().err
        assert "--echo" in err and s.split()[0] in err and "separate" in err
    for extra, word in ((["--echo_gain", "3"], "--echo"),                                # its option is refused without it
                        (["--project", "f.npz", "--echo_gain", "3"], "--echo"),
                        (["--echo", "e.npz", "--num", "4"], "--num"),                    # and the others' options with it
                        (["--echo", "e.npz", "--mask", "center:32"], "--inpaint"),
                        (["--echo", "e.npz", "--neighbours", "r.npz"], "--neighbours")):
        with pytest.raises(SystemExit):
            generate.get_arg_parse(BASE + extra)
        assert word in capsys.readouterr().err, extra
    with pytest.raises(SystemExit) as e:
        generate.get_arg_parse(["--help"])
    out = capsys.readouterr().out
    assert e.value.code == 0 and "echo (--echo)" in out and "--echo_gain" in out and echo_mode.doc in out
    for m in generate.MODES:                                                             # --help reads by mode
        assert f"{m.name} ({m.title()})" in out and m.doc in out


def test_the_table_is_as_it_was_without_the_added_mode():
    import generate
    assert [m.name for m in generate.MODES] == ["sample", "project", "inpaint", "anomaly", "features", "probe", "score_images"]
    with pytest.raises(SystemExit):
        generate.get_arg_parse(BASE + ["--echo", "e.npz"])
    for m in generate.MODES:
        assert m.doc in generate.__doc__
