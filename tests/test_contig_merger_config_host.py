"""parameters.contig_merger of the configuration JSON (main.parse_configuration) and the engine argument of MergeContigs.merge_contigs."""
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


def test_contig_merger_defaults_to_host(tmp_path):
    from gappadder_amd.main import parse_configuration
    assert parse_configuration(_config(tmp_path))["contig_merger"] == "host"


def test_contig_merger_accepts_device(tmp_path):
    from gappadder_amd.main import parse_configuration
    assert parse_configuration(_config(tmp_path, contig_merger="device"))["contig_merger"] == "device"
    assert parse_configuration(_config(tmp_path, contig_merger="host"))["contig_merger"] == "host"


def test_any_other_contig_merger_is_refused_by_name(tmp_path):
    from gappadder_amd.main import parse_configuration
    with pytest.raises(SystemExit) as e:
        parse_configuration(_config(tmp_path, contig_merger="gpu"))
    assert "contig_merger" in str(e.value)


def test_merge_contigs_refuses_an_unknown_engine_before_touching_a_file(tmp_path):
    from gappadder_amd import MergeContigs as MC
    d = tmp_path / "velvet_temp" / "g"
    d.mkdir(parents=True)
    (d / "contigs.fa").write_text(">a\nACGT\n")
    with pytest.raises(ValueError):
        MC.merge_contigs(None, str(tmp_path) + "/", ["g"], engine="bogus")
    assert sorted(x.name for x in d.iterdir()) == ["contigs.fa"] and (d / "contigs.fa").read_text() == ">a\nACGT\n"
