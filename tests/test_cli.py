"""The command line (genefuserust_amd/cli.py): the reference's options and defaults (src/argparse.rs), the checks in
front of the device, and — on the GPU, in a child process — the files and the text a run leaves."""
import os
import subprocess
import sys

import pytest

from tests.test_multi_csv_scan import _files

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "genefuserust_amd"] + list(args), cwd=str(cwd), env=env,
                          capture_output=True, text=True, timeout=300)


def test_the_reference_options_and_their_defaults():
    from genefuserust_amd.cli import parser
    a = parser().parse_args(["-1", "a.fq", "-f", "x.csv", "-r", "ref.fa"])
    assert (a.read1, a.read2, a.fusion, a.ref) == ("a.fq", "", "x.csv", "ref.fa")
    assert (a.unique, a.html, a.json, a.thread, a.deletion) == (2, "genefuse.html", "genefuse.json", 4, 50)
    assert a.output_deletions is False and a.output_untranslated_fusions is False
    assert (a.device, a.chunk_bytes, a.ref_chunk_bytes, a.inflate, a.tail, a.route, a.remove_alignables) == (
        -1, None, None, "host", "host", "device", False)
    # -h is the HTML file, not help
    a = parser().parse_args(["-1", "a.fq", "-2", "b.fq", "-f", "x.csv", "-r", "ref.fa", "-h", "out.html", "-j", "", "-u",
                             "3", "-d", "70", "-t", "8", "-D", "-U", "--chunk-bytes", "4096", "--tail", "device"])
    assert (a.html, a.json, a.read2, a.unique, a.deletion, a.thread) == ("out.html", "", "b.fq", 3, 70, 8)
    assert a.output_deletions and a.output_untranslated_fusions and a.chunk_bytes == 4096 and a.tail == "device"
    a = parser().parse_args(["--read1", "a.fq", "--fusion", "x.csv", "--ref", "r.fa", "--html", "", "--json", "j.json",
                             "--output_deletions", "--output_untranslated_fusions", "--remove-alignables"])
    assert (a.html, a.json) == ("", "j.json") and a.output_deletions and a.remove_alignables
    for missing in (["-f", "x.csv", "-r", "r.fa"], ["-1", "a.fq", "-r", "r.fa"], ["-1", "a.fq", "-f", "x.csv"]):
        with pytest.raises(SystemExit) as e:   # -1, -f and -r are required
            parser().parse_args(missing)
        assert e.value.code != 0


def test_help_is_the_long_option_only(capsys):
    from genefuserust_amd.cli import main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "-h HTML" in out and "--remove-alignables" in out and "removes nothing" in out and "panics" in out


def test_a_missing_input_file_ends_the_run_before_any_device_call(tmp_path, monkeypatch, capsys):
    from genefuserust_amd import cli, multi_csv_scan

    def boom(*a, **k):
        raise AssertionError("the scan was started")
    monkeypatch.setattr(multi_csv_scan, "scan_report", boom)
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", boom)
    for name in ("ref.fa", "x.csv"):
        (tmp_path / name).write_text("")
    gone = str(tmp_path / "gone.fq")
    rc = cli.main(["-1", gone, "-f", str(tmp_path / "x.csv"), "-r", str(tmp_path / "ref.fa")])
    captured = capsys.readouterr()
    assert rc != 0 and gone in captured.err and captured.out == ""
    # the same from a child process: a status, a message, no traceback, no files
    r = _run(["-1", gone, "-f", str(tmp_path / "x.csv"), "-r", str(tmp_path / "ref.fa")], tmp_path)
    assert r.returncode != 0 and gone in r.stderr and "Traceback" not in r.stderr
    assert not (tmp_path / "genefuse.html").exists() and not (tmp_path / "genefuse.json").exists()


def test_a_list_file_gets_its_reports_under_report_names(tmp_path, monkeypatch, capsys):
    """``-h`` and ``-j`` reach the scan as they are, for a list of CSVs too; the names per CSV are ``report_names``'."""
    from genefuserust_amd import cli, multi_csv_scan
    from genefuserust_amd.fusion_result import FusionResult
    seen = {}

    def scan_report(ref, fusion, r1, r2, **kw):
        seen.update(kw, fusion=fusion)
        for name in multi_csv_scan.report_names(kw["html_file"], ["/x/ab.csv", "/y/agr.csv"]):
            open(name, "w").write("page")
        return [("/x/ab.csv", [FusionResult(m_title="one")], {}), ("/y/agr.csv", [], {})]
    monkeypatch.setattr(multi_csv_scan, "scan_report", scan_report)
    for name in ("ref.fa", "panels.txt", "a.fq"):
        (tmp_path / name).write_text("")
    hf = str(tmp_path / "out.html")
    rc = cli.main(["-1", str(tmp_path / "a.fq"), "-f", str(tmp_path / "panels.txt"), "-r", str(tmp_path / "ref.fa"),
                   "-h", hf, "-j", "", "-D"])
    assert rc == 0 and seen["html_file"] == hf and seen["json_file"] == "" and seen["originals"] is True
    assert seen["settings"].output_deletions and seen["fusion"].endswith("panels.txt")
    assert sorted(os.listdir(tmp_path)) == ["a.fq", "out_ab.html", "out_agr.html", "panels.txt", "ref.fa"]
    out = capsys.readouterr().out
    assert out.startswith("\n# genefuserust_amd -1 ") and "\n#one\n" in out
    assert out.rstrip("\n").splitlines()[-1].startswith("# genefuse v")


def _outside(text: str, *line_starts):
    """``text`` without the lines that carry the time of the run."""
    return [ln for ln in text.split("\n") if not ln.startswith(line_starts)]


def _split_page(page: str):
    """(the page without its title and the footer's time, ...)."""
    head, rest = page.split("<title>", 1)
    rest = rest.split("</title>", 1)[1]
    body, tail = rest.rsplit(", at ", 1)
    assert tail.endswith(" </div></div></body></html>")
    return head + body


def _check_run(r, html, json_, want_html, want_json, want_text, args):
    from genefuserust_amd import __version__
    assert r.returncode == 0, r.stderr
    assert _split_page(open(html, encoding="utf-8").read()) == _split_page(want_html)
    assert _outside(open(json_).read(), "\t\"time\":") == _outside(want_json, "\t\"time\":")
    command = "genefuserust_amd " + " ".join(args)
    assert r.stdout.startswith("\n# %s\n\n" % command)
    assert want_text and want_text in r.stdout
    last = r.stdout[r.stdout.index(want_text) + len(want_text):]
    assert last.startswith("# genefuse v%s, time used: " % __version__) and last.endswith(" seconds\n\n")
    return command


@pytest.mark.gpu
def test_a_paired_run_in_a_child_process(gpu_device, tmp_path):
    from genefuserust_amd import __version__, report_html, report_json, report_text
    from genefuserust_amd.scan import scan_pair_end_report
    fa, _, csvs, r1, r2 = _files(tmp_path)
    html, json_ = str(tmp_path / "run.html"), str(tmp_path / "run.json")
    args = ["-1", r1, "-2", r2, "-f", csvs[3], "-r", fa, "-h", html, "-j", json_, "--chunk-bytes", "12000"]
    r = _run(args, tmp_path)
    results, counters = scan_pair_end_report(fa, csvs[3], r1, r2, originals=True, chunk_bytes=12000)
    assert counters["fusions"] >= 1
    command = "genefuserust_amd " + " ".join(args)
    _check_run(r, html, json_, report_html(results, command, __version__, "t"),
               report_json(results, command, __version__, "t"), report_text(results), args)
    assert "<xmp>@pair" in open(html, encoding="utf-8").read()


@pytest.mark.gpu
def test_a_single_end_run_in_a_child_process(gpu_device, tmp_path):
    from genefuserust_amd import __version__, report_html, report_json, report_text
    from genefuserust_amd.scan import scan_single_end_report
    fa, _, csvs, r1, _ = _files(tmp_path)
    # the default file names, in the working directory
    args = ["-1", r1, "-f", csvs[3], "-r", fa]
    r = _run(args, tmp_path)
    results, counters = scan_single_end_report(fa, csvs[3], r1, originals=True)
    assert counters["fusions"] >= 1
    command = "genefuserust_amd " + " ".join(args)
    _check_run(r, str(tmp_path / "genefuse.html"), str(tmp_path / "genefuse.json"),
               report_html(results, command, __version__, "t"), report_json(results, command, __version__, "t"),
               report_text(results), args)
