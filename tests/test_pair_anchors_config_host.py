"""parameters.fill_pairs_anchored and fill_pairs_min_pairs of the configuration JSON (main.parse_configuration; main exits with a message
on a value out of range, and on fill_pairs_anchored without fill_pairs)."""
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


def test_off_by_default_with_the_twins_default(tmp_path):
    from gappadder_amd import pair_anchors as PA
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path))
    assert cfg["fill_pairs_anchored"] is False and cfg["fill_pairs_min_pairs"] == PA.MIN_PAIRS == 8
    assert parse_configuration(_config(tmp_path, fill_pairs=True))["fill_pairs_anchored"] is False


def test_accepted_values(tmp_path):
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path, fill_pairs=True, fill_pairs_anchored=True))
    assert cfg["fill_pairs"] is True and cfg["fill_pairs_anchored"] is True and cfg["fill_pairs_min_pairs"] == 8
    for v in (1, 2, 8, 500):
        cfg = parse_configuration(_config(tmp_path, fill_pairs=True, fill_pairs_anchored=True, fill_pairs_min_pairs=v, fill_pairs_z=2))
        assert cfg["fill_pairs_min_pairs"] == v and cfg["fill_pairs_z"] == 2 and cfg["fill_pairs_seed"] == 16
    assert parse_configuration(_config(tmp_path, fill_pairs_min_pairs=3))["fill_pairs_min_pairs"] == 3       # read whether or not the round is on
    assert "fill_polish_min_pairs" not in cfg                                                                # the polish has no such option


@pytest.mark.parametrize("value", [0, -1, -8, "many"])
def test_a_value_out_of_range_makes_main_exit_with_a_message(tmp_path, value):
    from gappadder_amd import main as M
    cfgp = _config(tmp_path, fill_pairs=True, fill_pairs_anchored=True, fill_pairs_min_pairs=value)
    with pytest.raises(SystemExit) as e:
        M.parse_configuration(cfgp)
    assert "fill_pairs_min_pairs" in str(e.value)
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "Collect", "-g", cfgp])
    assert "fill_pairs_min_pairs" in str(e.value)


def test_anchored_without_fill_pairs_is_refused(tmp_path):
    from gappadder_amd import main as M
    for params in (dict(fill_pairs_anchored=True), dict(fill_pairs_anchored=True, fill_pairs=False, fill_polish=True)):
        cfgp = _config(tmp_path, **params)
        with pytest.raises(SystemExit) as e:
            M.parse_configuration(cfgp)
        assert "fill_pairs_anchored" in str(e.value) and "fill_pairs" in str(e.value)
        with pytest.raises(SystemExit):
            M.main(["-c", "Collect", "-g", cfgp])


def test_the_device_step_checks_the_parameters_against_the_libraries():
    """z * is_sd below 2^20, and min_pairs an integer: pair_anchors.check_params, which the device-resident Collect calls with the read
    length (device_collect.round_keywords)."""
    from gappadder_amd import device_collect as DC
    from gappadder_amd import pair_anchors as PA
    cfg = {"fill_pairs_seed": 16, "fill_pairs_max_mismatch": 4, "fill_pairs_min_overlap": 48, "fill_pairs_z": 3, "fill_pairs_min_pairs": 5}
    kw = DC.round_keywords(cfg, 150, "pairs", "pair", ("seed", "max_mismatch", "min_overlap", "z", "min_pairs"), PA.check_params, "pair_anchors")
    assert kw == {"pair_seed": 16, "pair_max_mismatch": 4, "pair_min_overlap": 48, "pair_z": 3, "pair_min_pairs": 5, "pair_anchors": True}
    with pytest.raises(SystemExit) as e:
        DC.round_keywords(dict(cfg, fill_pairs_min_overlap=151), 150, "pairs", "pair", ("seed", "max_mismatch", "min_overlap", "z", "min_pairs"),
                          PA.check_params, "pair_anchors")
    assert "fill_pairs_" in str(e.value)
