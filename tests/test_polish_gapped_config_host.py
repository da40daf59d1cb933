"""parameters.fill_polish_indels and fill_polish_max_indel of the configuration JSON (main.parse_configuration; main exits with a message
on a value out of range), and what Pipeline refuses before it touches the device."""
import json

import pytest


def _config(tmp_path, **params):
    for fn in ("d.fa", "a.bam", "l.fq", "r.fq"):
        (tmp_path / fn).write_text("")
    wf = tmp_path / "wf"
    wf.mkdir(exist_ok=True)
    p = tmp_path / "c.json"
    p.write_text(json.dumps({"draft_genome": {"fa": str(tmp_path / "d.fa")},
                             "alignments": [{"bam": str(tmp_path / "a.bam"), "is": 300, "std": 30}],
                             "raw_reads": [{"left": str(tmp_path / "l.fq"), "right": str(tmp_path / "r.fq")}],
                             "parameters": dict(params, working_folder=str(wf))}))
    return str(p)


def test_the_indel_mode_is_off_by_default_with_the_twins_default():
    from gappadder_amd import polish_gapped as PG
    assert PG.MAX_INDEL == 8


def test_defaults_and_values_are_read(tmp_path):
    from gappadder_amd import polish_gapped as PG
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path))
    assert cfg["fill_polish_indels"] is False and cfg["fill_polish_max_indel"] == PG.MAX_INDEL == 8
    cfg = parse_configuration(_config(tmp_path, fill_polish=True))
    assert cfg["fill_polish"] is True and cfg["fill_polish_indels"] is False
    cfg = parse_configuration(_config(tmp_path, fill_polish=True, fill_polish_indels=True, fill_polish_max_indel=16))
    assert cfg["fill_polish_indels"] is True and cfg["fill_polish_max_indel"] == 16
    assert parse_configuration(_config(tmp_path, fill_polish=True, fill_polish_indels=True, fill_polish_max_indel=1))["fill_polish_max_indel"] == 1


@pytest.mark.parametrize("params,name", [({"fill_polish": True, "fill_polish_indels": True, "fill_polish_max_indel": 0}, "fill_polish_max_indel"),
                                         ({"fill_polish": True, "fill_polish_indels": True, "fill_polish_max_indel": 17}, "fill_polish_max_indel"),
                                         ({"fill_polish": True, "fill_polish_indels": True, "fill_polish_max_indel": "long"}, "fill_polish_max_indel"),
                                         ({"fill_polish_indels": True}, "fill_polish_indels")])
def test_a_value_out_of_range_makes_main_exit_with_a_message(tmp_path, params, name):
    from gappadder_amd import main as M
    cfgp = _config(tmp_path, **params)
    with pytest.raises(SystemExit) as e:
        M.parse_configuration(cfgp)
    assert name in str(e.value)
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "Collect", "-g", cfgp])
    assert name in str(e.value)


def test_pipeline_refuses_the_mode_without_the_round_and_a_length_out_of_range():
    """The refusals come before anything touches the device or the library: no GapFill is needed."""
    from gappadder_amd.pipeline import Pipeline
    with pytest.raises(ValueError, match="polish_indels needs polish"):
        Pipeline(None, 24, 150, [(31, 29)], polish_indels=True)
    with pytest.raises(ValueError, match="second_round"):
        Pipeline(None, 24, 150, [(31, 29)], polish=True, polish_indels=True, second_round=True)
    with pytest.raises(ValueError, match="single rank"):
        Pipeline(None, 24, 150, [(31, 29)], polish=True, polish_indels=True, world=2)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="max_indel"):
            Pipeline(None, 24, 150, [(31, 29)], polish=True, polish_indels=True, polish_max_indel=bad)


def test_the_collectors_keywords(tmp_path):
    from gappadder_amd import polish_gapped as PG
    from gappadder_amd.device_collect import round_keywords
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path, fill_polish=True, fill_polish_indels=True, fill_polish_max_indel=5, fill_polish_seed=20))
    kw = round_keywords(cfg, 150, "polish", "polish", ("seed", "max_mismatch", "min_overlap", "min_votes", "max_indel"), PG.check_params, "polish")
    assert kw == dict(polish=True, polish_seed=20, polish_max_mismatch=4, polish_min_overlap=48, polish_min_votes=2, polish_max_indel=5)
