"""parameters.fill_polish and its four optional parameters of the configuration JSON (main.parse_configuration; main exits with a
message on a value out of range)."""
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


def test_fill_polish_is_off_by_default_with_the_twins_defaults(tmp_path):
    from gappadder_amd import polish as PL
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path))
    assert cfg["fill_polish"] is False
    assert (cfg["fill_polish_seed"], cfg["fill_polish_max_mismatch"], cfg["fill_polish_min_overlap"], cfg["fill_polish_min_votes"]) \
        == (PL.SEED, PL.MAX_MISMATCH, PL.MIN_OVERLAP, PL.MIN_VOTES) == (16, 4, 48, 2)


def test_fill_polish_and_its_parameters_are_read(tmp_path):
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path, fill_polish=True, fill_polish_seed=20, fill_polish_max_mismatch=3, fill_polish_min_overlap=60,
                                      fill_polish_min_votes=3))
    assert cfg["fill_polish"] is True
    assert (cfg["fill_polish_seed"], cfg["fill_polish_max_mismatch"], cfg["fill_polish_min_overlap"], cfg["fill_polish_min_votes"]) == (20, 3, 60, 3)
    edge = parse_configuration(_config(tmp_path, fill_polish_seed=12, fill_polish_max_mismatch=0, fill_polish_min_overlap=12, fill_polish_min_votes=1))
    assert (edge["fill_polish_seed"], edge["fill_polish_max_mismatch"], edge["fill_polish_min_overlap"], edge["fill_polish_min_votes"]) == (12, 0, 12, 1)
    assert parse_configuration(_config(tmp_path, fill_polish_seed=32, fill_polish_max_mismatch=15))["fill_polish_seed"] == 32


@pytest.mark.parametrize("params,name", [({"fill_polish_seed": 11}, "fill_polish_seed"), ({"fill_polish_seed": 33}, "fill_polish_seed"),
                                         ({"fill_polish_max_mismatch": -1}, "fill_polish_max_mismatch"),
                                         ({"fill_polish_max_mismatch": 16}, "fill_polish_max_mismatch"),
                                         ({"fill_polish_min_overlap": 15}, "fill_polish_min_overlap"),
                                         ({"fill_polish_seed": 12, "fill_polish_min_overlap": 11}, "fill_polish_min_overlap"),
                                         ({"fill_polish_min_votes": 0}, "fill_polish_min_votes"), ({"fill_polish_seed": "long"}, "fill_polish_seed")])
def test_a_value_out_of_range_makes_main_exit_with_a_message(tmp_path, params, name):
    from gappadder_amd import main as M
    cfgp = _config(tmp_path, fill_polish=True, **params)
    with pytest.raises(SystemExit) as e:
        M.parse_configuration(cfgp)
    assert name in str(e.value)
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "Collect", "-g", cfgp])
    assert name in str(e.value)
