"""CPU tier: main.py, batch_main.py, request_settings and DecodeEngine.generate make of their arguments what they made before the request
settings got one table (tiny_llm_hip/request.py), and the table is the one declaration.

tests/golden/request_cli.json holds both scripts' parser surface, the outcome of every command line of tests/request_cli_recorder.py
(the refusal's text; or the entry points reached with their arguments, every engine's settings calls with their values and the digest of its whole call
log, the notes and the printed text) and the outcome of every ``sampling`` argument there through request_settings and through generate(**kw), written by
tests/golden/make_request_cli.py at the commit the file names.  It is never regenerated from the code under test."""

import json
from pathlib import Path

import pytest

import request_cli_recorder as R

GOLDEN = json.loads((Path(__file__).parent / "golden" / "request_cli.json").read_text())
MAIN, BATCH, SETTINGS, GENERATE = R.main_vectors(), R.batch_vectors(), R.settings_cases(), R.generate_cases()
MATCHED = "stop id matched"  # (request_cli_recorder.run_matched_stop)


def test_the_fixture_covers_every_scenario_and_names_its_commit():
    assert sorted(GOLDEN["main"]) == sorted([*MAIN, MATCHED]) and sorted(GOLDEN["batch_main"]) == sorted([*BATCH, MATCHED])
    assert sorted(GOLDEN["settings"]) == sorted(SETTINGS) and sorted(GOLDEN["generate"]) == sorted(GENERATE)
    assert len(GOLDEN["commit"]) == 40


# ---- A. equivalence with the commit the fixture names ---------------------------------------------------------------------------------
@pytest.mark.parametrize("script", ["main", "batch_main"])
def test_parser_surface_is_the_pinned_one(script):
    got, want = R.parser_surface(script), GOLDEN["parsers"][script]
    assert sorted(got) == sorted(want)
    for option in want:
        assert got[option] == want[option], option


def _same_outcome(got, section, name):
    want = GOLDEN["pool"][GOLDEN[section][name]]
    assert got["error"] == want["error"]
    for key in want:
        assert got[key] == want[key], key
    assert sorted(got) == sorted(want)


@pytest.mark.parametrize("name", sorted(MAIN))
def test_main_outcome_is_the_pinned_one(name):
    _same_outcome(R.run_cli("main", MAIN[name]), "main", name)


@pytest.mark.parametrize("name", sorted(BATCH))
def test_batch_main_outcome_is_the_pinned_one(name):
    _same_outcome(R.run_cli("batch_main", BATCH[name]), "batch_main", name)


@pytest.mark.parametrize("script", ["main", "batch_main"])
def test_outcome_with_a_stop_set_that_matches_is_the_pinned_one(script):
    _same_outcome(R.run_matched_stop(script), script, MATCHED)


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_request_settings_outcome_is_the_pinned_one(name):
    _same_outcome(R.run_settings(SETTINGS[name]), "settings", name)


@pytest.mark.parametrize("name", sorted(GENERATE))
def test_generate_outcome_is_the_pinned_one(name):
    _same_outcome(R.run_generate(GENERATE[name]), "generate", name)


def test_generate_refuses_an_unknown_keyword_as_request_settings_does():
    got = R.run_generate({"temp": 1.0})
    assert got["error"] == "ValueError: unknown sampling keys: ['temp']" and got["calls"] == R.engine_log([])


# ---- B. the table is the one declaration ----------------------------------------------------------------------------------------------
def test_the_keys_and_the_neutral_record_follow_from_the_table():
    from tiny_llm_hip import request
    from tiny_llm_hip.engine import DRY_OFF, SETTINGS_KEYS, RequestSettings, request_settings

    assert SETTINGS_KEYS == {s.key for s in request.SETTINGS} and len(request.SETTINGS) == len(SETTINGS_KEYS) == 20
    assert request_settings(None, 1)[0] == RequestSettings()
    assert RequestSettings().dry == DRY_OFF
    assert {s.group for s in request.SETTINGS} == {"sampling", "truncation", "penalties", "bias", "dry", "grammar", "lora"}


def _options(parser):
    return {a.option_strings[0]: a for a in parser._actions if a.dest != "help"}


def test_every_flag_of_the_table_is_in_both_parsers_as_declared():
    import batch_main
    import main
    from tiny_llm_hip import request

    parsers = {"main": _options(main.build_parser()), "batch_main": _options(batch_main.build_parser())}
    declared = [(s, f) for s in request.SETTINGS for f in s.flags] + [(None, f) for f in request.STOP_FLAGS]
    for script, options in parsers.items():
        for setting, flag in declared:
            action = options[flag.option]
            assert action.type is flag.kw.get("type") and action.dest == flag.dest, flag.option
            default = setting.default if setting is not None else ()
            if flag.option == "--sampler-seed":  # the one declared per-script default
                assert flag.defaults == {"main": None, "batch_main": 0}
                default = flag.defaults[script]
            else:
                assert not flag.defaults, flag.option
            # (a repeatable flag collects into a list: an empty one for the table's empty tuple)
            assert action.default == (list(default) if flag.kw.get("action") == "append" else default), flag.option
            assert type(action.default) is type(list(default) if flag.kw.get("action") == "append" else default), flag.option
    # what the two scripts share: the table's flags, the two stop flags declared beside it, four plain ones -- and the name of --lora,
    # which is each script's own flag (one adapter there, several here)
    shared = set(parsers["main"]) & set(parsers["batch_main"])
    assert shared == {f.option for _, f in declared} | {"--model", "--draft-model", "--proposal-length", "--enable-thinking", "--lora"}
    assert type(parsers["main"]["--lora"]) is not type(parsers["batch_main"]["--lora"])
    assert {f.option for f in request.STOP_FLAGS} == {"--stop", "--stop-id"}


def test_given_and_on_are_two_questions():
    """--sampler-typical-p 1.0 is given (what --num-beams refuses) and off (no truncation, no clash with Mirostat)."""
    import main
    from tiny_llm_hip import request

    flags = request.switched(main.build_parser().parse_args(["--model", "m", "--sampler-typical-p", "1.0", "--sampler-top-k", "40", "--dry-base", "3"]))
    assert flags.given == {"--sampler-typical-p", "--sampler-top-k"} and flags.on == {"--sampler-top-k"} and flags.groups == set()
    flags = request.switched(main.build_parser().parse_args(["--model", "m", "--sampler-temp", "0.5", "--stop-id", "3", "--json", "value", "--presence-penalty", "-1"]))
    assert flags.groups == {"sampling", "stop", "grammar", "penalties"}
