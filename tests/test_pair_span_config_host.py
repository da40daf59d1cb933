"""parameters.fill_pairs and its four optional parameters of the configuration JSON (main.parse_configuration; main exits with a
message on a value out of range)."""
import json

import pytest

KEYS = ("fill_pairs_seed", "fill_pairs_max_mismatch", "fill_pairs_min_overlap", "fill_pairs_z")


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


def test_fill_pairs_is_off_by_default_with_the_twins_defaults(tmp_path):
    from gappadder_amd import pair_span as PS
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path))
    assert cfg["fill_pairs"] is False
    assert tuple(cfg[k] for k in KEYS) == (PS.SEED, PS.MAX_MISMATCH, PS.MIN_OVERLAP, PS.Z) == (16, 4, 48, 3)


def test_fill_pairs_and_its_parameters_are_read(tmp_path):
    from gappadder_amd.main import parse_configuration
    cfg = parse_configuration(_config(tmp_path, fill_pairs=True, fill_pairs_seed=20, fill_pairs_max_mismatch=3, fill_pairs_min_overlap=60, fill_pairs_z=2))
    assert cfg["fill_pairs"] is True and tuple(cfg[k] for k in KEYS) == (20, 3, 60, 2)
    edge = parse_configuration(_config(tmp_path, fill_pairs_seed=12, fill_pairs_max_mismatch=0, fill_pairs_min_overlap=12, fill_pairs_z=1))
    assert tuple(edge[k] for k in KEYS) == (12, 0, 12, 1)
    assert parse_configuration(_config(tmp_path, fill_pairs_seed=32, fill_pairs_max_mismatch=15))["fill_pairs_seed"] == 32
    both = parse_configuration(_config(tmp_path, fill_pairs=True, fill_polish=True, fill_polish_seed=20))       # the polish's options are its own
    assert both["fill_pairs_seed"] == 16 and both["fill_polish_seed"] == 20


@pytest.mark.parametrize("params,name", [({"fill_pairs_seed": 11}, "fill_pairs_seed"), ({"fill_pairs_seed": 33}, "fill_pairs_seed"),
                                         ({"fill_pairs_max_mismatch": -1}, "fill_pairs_max_mismatch"),
                                         ({"fill_pairs_max_mismatch": 16}, "fill_pairs_max_mismatch"),
                                         ({"fill_pairs_min_overlap": 15}, "fill_pairs_min_overlap"),
                                         ({"fill_pairs_seed": 12, "fill_pairs_min_overlap": 11}, "fill_pairs_min_overlap"),
                                         ({"fill_pairs_z": 0}, "fill_pairs_z"), ({"fill_pairs_z": -3}, "fill_pairs_z"),
                                         ({"fill_pairs_seed": "long"}, "fill_pairs_seed")])
def test_a_value_out_of_range_makes_main_exit_with_a_message(tmp_path, params, name):
    from gappadder_amd import main as M
    cfgp = _config(tmp_path, fill_pairs=True, **params)
    with pytest.raises(SystemExit) as e:
        M.parse_configuration(cfgp)
    assert name in str(e.value)
    with pytest.raises(SystemExit) as e:
        M.main(["-c", "Collect", "-g", cfgp])
    assert name in str(e.value)
