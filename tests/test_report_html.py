"""``report_html`` (genefuserust_amd/fusion_result.py) against bytes written out by hand from the reference's source:
html_reporter.rs:195-364, read_match.rs:92-120, read.rs:127-165 / :199-213 / :263-297, fusion_result.rs:462-759.
No device: the reporter is host code."""
import pytest

from genefuserust_amd import GenePos, ReadMatch
from genefuserust_amd.fusion_result import (FusionResult, Settings, html_body, html_original_reads, html_protein,
                                            html_read_row, quality_color, report_html)
from genefuserust_amd.indexer import Gene

RIGHT, LEFT, DOWN = "→", "←", "↓"


def gene(name: str, n_exons: int, reversed_: bool = False) -> Gene:
    g = Gene(name, "chr1", 1000, 1000 + 1000 * n_exons)
    order = range(n_exons, 0, -1) if reversed_ else range(1, n_exons + 1)
    for k, pos in zip(range(1, n_exons + 1), order):
        g.add_exon(k, 1000 * pos, 1000 * pos + 500)
    assert g.is_reversed() == (reversed_ and n_exons > 1)
    return g


def result(left, right, matches=(), title="T", contigs=(0, 1)) -> FusionResult:
    """left / right: (gene, gene position, is_exon, exon or intron number)."""
    return FusionResult(m_left_gp=GenePos(contigs[0], left[1]), m_right_gp=GenePos(contigs[1], right[1]),
                        m_matches=list(matches), m_unique=len(matches), m_title=title, m_left_ref=b"ACGT",
                        m_right_ref=b"TTGA", m_left_ref_ext=b"ACGTAA", m_right_ref_ext=b"CCTTGA", m_left_pos="L:pos",
                        m_right_pos="R:pos", m_left_gene=left[0], m_right_gene=right[0], m_left_is_exon=left[2],
                        m_right_is_exon=right[2], m_left_exon_or_intron_id=left[3], m_right_exon_or_intron_id=right[3])


def match(name=b"@r1/1", seq=b"ACGTA", qual=b"I?50/", brk=1, reversed_=False, originals=()) -> ReadMatch:
    return ReadMatch(seq, brk, GenePos(0, 100), GenePos(1, 200), 0, 1, 2, reversed_, name, m_quality=qual,
                     m_original_reads=list(originals))


def td(style, width, text):
    return "<td class='%s' width='%d%%'>%s</td>" % (style, width, text)


def protein(lp, rp, lname, rname, left_cells, right_cells):
    """fusion_result.rs:543-574 around the cells: note the left percentage on the protein_right cell."""
    inner = "<table width='100%' class='protein_table'>\n<tr>"
    return ("<table width='100%' class='protein_table'>\n<tr>" + "<td width='%d%%'>%s</td><td width='%d%%'>%s</td></tr>" %
            (lp, lname, rp, rname) + "<tr><td class='protein_left' width='%d%%'>" % lp + inner + "".join(left_cells) +
            "</tr></table></td><td class='protein_right' width='%d%%'>" % lp + inner + "".join(right_cells) +
            "</tr></table></td></tr></table>")


def test_quality_color_at_its_thresholds():
    want = {"/": "#FF0000", "0": "#E99E5B", "4": "#E99E5B", "5": "#666666", ">": "#666666", "?": "#33BBE2",
            "H": "#33BBE2", "I": "#78C6B9"}
    assert {c: quality_color(ord(c)) for c in want} == want


def base(q, color, b):
    return "<a title='%s'><font color='%s'>%s</font></a>" % (q, color, b)


def test_a_row():
    # the break in the middle: bases 0..1 right-aligned, the rest left-aligned; the stray </span> of read_match.rs:101
    left = base("I", "#78C6B9", "A") + base("?", "#33BBE2", "C")
    right = base("5", "#666666", "G") + base("0", "#E99E5B", "T") + base("/", "#FF0000", "A")
    assert html_read_row(match(), 1) == (
        "<td><a title='@r1/1'>0001" + RIGHT + "</a></span></td><td>1|2</td><td class='alignright'>" + left +
        "</td><td class='alignleft'>" + right + "</td>")
    # a read found on the reverse complement; nothing is escaped
    assert html_read_row(match(name=b"@<r>&'2", reversed_=True), 12).startswith(
        "<td><a title='@<r>&'2'>0012" + LEFT + "</a></span></td><td>1|2</td>")
    # a break of -1: read_break + 1 is not > 0, and the right cell is not written
    assert html_read_row(match(brk=-1), 3) == (
        "<td><a title='@r1/1'>0003" + RIGHT + "</a></span></td><td>1|2</td><td class='alignright'></td>")
    # the break at the last base: an empty right cell
    assert html_read_row(match(brk=4), 3).endswith(base("/", "#FF0000", "A") + "</td><td class='alignleft'></td>")
    for number, text in ((9, "0009"), (10, "0010"), (99, "0099"), (100, "0100"), (999, "0999"), (1000, "1000")):
        assert html_read_row(match(), number).startswith("<td><a title='@r1/1'>" + text + RIGHT + "</a>")
    with pytest.raises(IndexError):   # quality.get(i..i+1).unwrap() of a quality shorter than the read
        html_read_row(match(qual=b"II"), 1)


R1 = (b"@p7/1", b"ACGTACGT", b"+", b"FFFFFFFF")
R2 = (b"@p7/2", b"TTGACA", b"+", b"FF#FFF")


def test_hidden_rows():
    assert html_original_reads(match()) == ""
    assert html_original_reads(match(originals=[R1])) == "@p7/1\nACGTACGT\n+\nFFFFFFFF\n"
    assert html_original_reads(match(originals=[R1, R2])) == "@p7/1\nACGTACGT\n+\nFFFFFFFF\n@p7/2\nTTGACA\n+\nFF#FFF\n"
    assert html_original_reads(match(originals=[(b"@cut", b"AC", b"", b"")])) == "@cut\nAC\n\n\n"


# -- the diagram: every side x direction x exon / intron, cells written out from fusion_result.rs:579-725 ---------------

def test_diagram_left_forward_exon_right_forward_intron_and_a_half_percent():
    """Left: exon 1 of a forward gene, 0.5 + 0 steps.  Right: intron 1 of three exons, 2 + 1.5 steps.
    0.5 * 100 / 4 = 12.5 rounds away from zero to 13 (Python's round gives 12)."""
    fr = result((gene("GL", 3), 50, True, 1), (gene("GRT", 3), 1700, False, 1))
    assert fr.is_left_protein_forward() and fr.is_right_protein_forward()
    assert html_protein(fr) == protein(13, 87, "GL", "GRT", [td("exon_left", 100, "E1")], [
        td("intron_right", 14, RIGHT), td("exon_right", 28, "E2"), td("intron_right", 28, RIGHT),
        td("exon_right", 28, "E3")])


def test_diagram_left_forward_intron_right_reversed_exon():
    """Left: intron 2, 2 + 1.5 steps of 28.57 %, the last a half.  Right: a forward gene met on its other strand
    (position < 0), exon 2: 1.5 + 1 steps of 40 %, the first a half, counting down.  3.5 * 100 / 6 = 58.33."""
    fr = result((gene("GL", 3), 2700, False, 2), (gene("GRT", 3), -2100, True, 2))
    assert fr.is_left_protein_forward() and not fr.is_right_protein_forward()
    assert html_protein(fr) == protein(58, 42, "GL", "GRT", [
        td("exon_left", 28, "E1"), td("intron_left", 28, RIGHT), td("exon_left", 28, "E2"), td("intron_left", 14, RIGHT)], [
        td("exon_right", 20, "E2"), td("intron_right", 40, LEFT), td("exon_right", 40, "E1")])


def test_diagram_left_reversed_exon_right_forward_exon():
    """Left: a reversed gene at a positive position (protein not forward), exon 2 of 3: (3 - 2) + 0.5 exons and
    (2 - 2) + 1 introns, from E3 down.  Right: a reversed gene at a negative position (forward), exon 2: the same
    sizes, from E2 up.  50 % each."""
    fr = result((gene("GL", 3, True), 2100, True, 2), (gene("GRT", 3, True), -2100, True, 2))
    assert not fr.is_left_protein_forward() and fr.is_right_protein_forward()
    assert html_protein(fr) == protein(50, 50, "GL", "GRT", [
        td("exon_left", 40, "E3"), td("intron_left", 40, LEFT), td("exon_left", 20, "E2")], [
        td("exon_right", 20, "E2"), td("intron_right", 40, RIGHT), td("exon_right", 40, "E3")])


def test_diagram_left_reversed_intron_right_reversed_intron():
    """Left: intron 1 of 3 exons, not forward: 2 + 1.5 steps from E3 down.  Right: intron 2, not forward: 2 + 1.5 steps,
    the half intron first, the exon number not advanced by it (fusion_result.rs:685-690)."""
    fr = result((gene("GL", 3), -1700, False, 1), (gene("GRT", 3), -2700, False, 2))
    assert not fr.is_left_protein_forward() and not fr.is_right_protein_forward()
    assert html_protein(fr) == protein(50, 50, "GL", "GRT", [
        td("exon_left", 28, "E3"), td("intron_left", 28, LEFT), td("exon_left", 28, "E2"), td("intron_left", 14, LEFT)], [
        td("intron_right", 14, LEFT), td("exon_right", 28, "E2"), td("intron_right", 28, LEFT),
        td("exon_right", 28, "E1")])


def test_diagram_cells_below_one_percent_become_one():
    """Left: exon 26 of 60: 25.5 + 25 steps of 1.98 % (1 as i32); the last, half exon 0.99 % -> 0 -> 1.
    Right: exon 1, not forward: 0.5 + 0 steps.  50.5 * 100 / 51 = 99.02."""
    fr = result((gene("GL", 60), 50, True, 26), (gene("GRT", 2), -50, True, 1))
    cells = []
    for k in range(1, 26):
        cells += [td("exon_left", 1, "E%d" % k), td("intron_left", 1, RIGHT)]
    cells.append(td("exon_left", 1, "E26"))
    assert html_protein(fr) == protein(99, 1, "GL", "GRT", cells, [td("exon_right", 100, "E1")])


def test_diagram_of_a_gene_without_exons_raises():
    with pytest.raises(IndexError):   # total_exon - 1 underflows a usize in the reference
        html_protein(result((gene("GL", 0), 50, True, 1), (gene("GRT", 3), 50, True, 1)))


# -- the page -----------------------------------------------------------------------------------------------------

HELPER = (
    "<div id='helper'><p>Helpful tips:</p><ul><li> Base color indicates quality: <font color='#78C6B9'>extremely high "
    "(Q40+)</font>, <font color='#33BBE2'>high (Q30~Q39) </font>, <font color='#666666'>moderate (Q20~Q29)</font>, "
    "<font color='#E99E5B'>low (Q15~Q19)</font>, <font color='#FF0000'>extremely low (0~Q14).</font> </li><li> Move "
    "mouse over the base, it will show the quality value</li><li> Click on any row, the original read/pair will be "
    "displayed</li><li> For pair-end sequencing, GeneFuse tries to merge each pair, with overlapped assigned higher "
    "qualities </li></ul><p>Columns:</p><ul><li> col1: is fusion mapped with original read? " + RIGHT + " means "
    "original read, " + LEFT + " means reverse complement</li><li> col2: edit distance (ed) between read and reference "
    "sequence (left_part_ed | right_part_ed)</li><li> col3: read's left part after fusion break</li><li> col4: read's "
    "right part after fusion break</li></ul></div>")
SOFTWARE = ("<body><div id='container'><div class='software'> <a href='https://github.com/OpenGene/GeneFuse' "
            "style='text-decoration:none;' target='_blank'>GeneFuse</a> <font size='-1'>0.8.0</font></div>")
FOOTER = "<div id='footer'> <p>genefuse -1 a.fq</p>GeneFuse 0.8.0, at 2024-01-02 03:04:05 </div></div></body></html>"


def _three_results():
    a = result((gene("GL", 3), 50, True, 1), (gene("GRT", 3), 1700, False, 1), title="Fusion: A",
               matches=[match(originals=[R1, R2]), match(name=b"@r2/1", reversed_=True, originals=[R1])])
    deletion = result((gene("GL", 3), 50, True, 1), (gene("GL", 3), 1700, False, 1), title="Deletion: B",
                      matches=[match()], contigs=(0, 0))
    c = result((gene("GL", 3), -1700, False, 1), (gene("GRT", 3), -2700, False, 2), title="Fusion: C",
               matches=[match(name=b"@r3/1")])
    assert deletion.is_deletion() and not a.is_deletion() and not c.is_deletion()
    return [a, deletion, c]


def _block(id_, fr, proteins, rows):
    """html_reporter.rs:288-361 around the diagram and the rows."""
    return ("<div class='fusion_block'><div class='fusion_head'><a name='fusion_id_%d'>%d, %s</a></div>" %
            (id_, id_, fr.m_title) + "<div class='tips'>Inferred protein:</div>" + proteins +
            "<div class='tips'>Supporting reads:</div><table><tr class='header'>"
            "<td class='alignright' colspan='3'>L:pos = <font color='yellow'>" + DOWN + "</font></td>"
            "<td class='alignleft'><font color='yellow'>" + DOWN + "</font> = R:pos</td></tr><tr class='header'>"
            "<td class='alignright' colspan='3'><a title='ACGT___ACGTAA'>ACGT</a></td>"
            "<td class='alignleft'><a title='CCTTGA___TTGA'>TTGA</a></td></tr>" + "".join(rows) + "</table></div>")


def _row(rowid, name, number, arrow, hidden):
    left = base("I", "#78C6B9", "A") + base("?", "#33BBE2", "C")
    right = base("5", "#666666", "G") + base("0", "#E99E5B", "T") + base("/", "#FF0000", "A")
    return ("<tr onclick='toggle(%d);'><td><a title='%s'>%s%s</a></span></td><td>1|2</td><td class='alignright'>%s</td>"
            "<td class='alignleft'>%s</td></tr><tr id='%d' style='display:none;'><td colspan='6'><xmp>%s</xmp></td></tr>" %
            (rowid, name, number, arrow, left, right, rowid, hidden))


def test_the_body_menu_numbers_every_result_and_the_blocks_their_own():
    results = _three_results()
    body = html_body(results, "genefuse -1 a.fq", "0.8.0", "2024-01-02 03:04:05")
    menu = ("<div id='menu'><p>Found 3 fusions:</p><ul>"
            "<li class='menu_item'><a href='#fusion_id_1'> 1, Fusion: A</a></li>"
            "<li class='menu_item'><a href='#fusion_id_2'> 2, Deletion: B</a></li>"
            "<li class='menu_item'><a href='#fusion_id_3'> 3, Fusion: C</a></li></ul></div>")
    block_a = _block(1, results[0], protein(13, 87, "GL", "GRT", [td("exon_left", 100, "E1")], [
        td("intron_right", 14, RIGHT), td("exon_right", 28, "E2"), td("intron_right", 28, RIGHT),
        td("exon_right", 28, "E3")]), [
        _row(100000, "@r1/1", "0001", RIGHT, "@p7/1\nACGTACGT\n+\nFFFFFFFF\n@p7/2\nTTGACA\n+\nFF#FFF\n"),
        _row(100001, "@r2/1", "0002", LEFT, "@p7/1\nACGTACGT\n+\nFFFFFFFF\n")])
    # the deletion is in the menu as number 2 and has no block; the third result's block is number 2
    block_c = _block(2, results[2], protein(50, 50, "GL", "GRT", [
        td("exon_left", 28, "E3"), td("intron_left", 28, LEFT), td("exon_left", 28, "E2"), td("intron_left", 14, LEFT)], [
        td("intron_right", 14, LEFT), td("exon_right", 28, "E2"), td("intron_right", 28, LEFT),
        td("exon_right", 28, "E1")]), [_row(200000, "@r3/1", "0001", RIGHT, "")])
    assert body == SOFTWARE + HELPER + menu + block_a + block_c + FOOTER
    # with deletions asked for, the block is there and the numbers agree
    with_deletions = html_body(results, "genefuse -1 a.fq", "0.8.0", "2024-01-02 03:04:05",
                               Settings(output_deletions=True))
    assert "<a name='fusion_id_2'>2, Deletion: B</a>" in with_deletions
    assert "<a name='fusion_id_3'>3, Fusion: C</a>" in with_deletions and "toggle(300000)" in with_deletions


def test_the_body_of_one_and_of_no_fusion_and_a_direction_conflict():
    assert html_body([], "c", "0.8.0", "t") == (
        SOFTWARE + HELPER + "<div id='menu'><p>Found 0 fusion:</p><ul></ul></div>"
        "<div id='footer'> <p>c</p>GeneFuse 0.8.0, at t </div></div></body></html>")
    conflict = result((gene("GL", 3), 2700, False, 2), (gene("GRT", 3), -2100, True, 2), title="Fusion: X")
    body = html_body([conflict], "c", "0.8.0", "t")
    assert "<p>Found 1 fusion:</p>" in body and "fusion_id_1'> 1, Fusion: X</a>" in body
    assert "fusion_block" not in body            # listed, but not drawn
    body = html_body([conflict], "c", "0.8.0", "t", Settings(output_untranslated=True))
    assert ("<div class='tips'>Inferred protein (transcription direction conflicts, this fusion may be not transcribed) "
            ":</div>") in body


def test_the_head_has_a_toggle_and_the_body_does_not_change_with_it():
    results = _three_results()
    page = report_html(results, "genefuse -1 a.fq", "0.8.0", "2024-01-02 03:04:05")
    head, body = page[:page.index("<body>")], page[page.index("<body>"):]
    assert body == html_body(results, "genefuse -1 a.fq", "0.8.0", "2024-01-02 03:04:05")
    assert head.startswith("<html><head><meta http-equiv=\"content-type\" content=\"text/html;charset=utf-8\" />"
                           "<title>GeneFuse 0.8.0, at 2024-01-02 03:04:05</title>") and head.endswith("</head>")
    assert "function toggle(" in head and "table-row" in head and "<script" in head and "<style" in head
    for name in (".alignleft", ".alignright", ".software", ".header", "#menu", ".menu_item", ".fusion_head",
                 ".fusion_block", ".tips", "#helper", "#footer", ".protein_table", ".exon_left", ".exon_right",
                 ".intron_left", ".intron_right", "#container"):
        assert name in head, name
    assert "toggle(" not in body.replace("onclick='toggle(", "")   # the body only calls it


def test_the_page_of_clustered_planted_matches():
    """Real results — planted reads across two junctions, clustered on the host — go through the reporter: every result
    in the menu, a block and one row pair per supporting read, the originals in the hidden rows."""
    import numpy as np
    from genefuserust_amd import Fusion
    from genefuserust_amd.fusion_result import cluster_matches, group_and_sort
    from tests.helpers import rand_seq
    from tests.test_fusion_result import CSV, planted_matches
    rng = np.random.default_rng(11)
    fusions = Fusion.parse_csv_text(CSV)
    seqs = [rand_seq(rng, 6000), rand_seq(rng, 6000), rand_seq(rng, 5000)]
    ms = planted_matches(rng, seqs, 0, 1500, 1, 2600, 6) + planted_matches(rng, seqs, 0, 2500, 2, -1200, 5)
    for k, m in enumerate(ms):
        m.m_original_reads = [(m.m_name, m.m_read, b"+", m.m_quality), (b"@mate%d/2" % k, b"ACGT", b"+", b"FFFF")]
    results = cluster_matches(group_and_sort(ms, len(fusions)), fusions, [s.decode() for s in seqs],
                              Settings(output_untranslated=True))
    assert len(results) == 2
    settings = Settings(output_untranslated=True)
    page = report_html(results, "cmd", "0.1.0", "now", settings)
    assert "<p>Found 2 fusions:</p>" in page and page.count("<div class='fusion_block'>") == 2
    n = sum(len(fr.m_matches) for fr in results)
    assert n == 11 and page.count("<tr onclick='toggle(") == n == page.count("<xmp>@read")
    for k, fr in enumerate(results):
        assert "<a name='fusion_id_%d'>%d, %s</a>" % (k + 1, k + 1, fr.m_title) in page
        for m in fr.m_matches:   # (a refined break keeps the records of its match)
            assert len(m.m_original_reads) == 2 and m.m_original_reads[0][0] == m.m_name
            assert "<xmp>%s\n%s\n+\n%s\n@mate" % (m.m_name.decode(), m.m_original_reads[0][1].decode(),
                                                 m.m_original_reads[0][3].decode()) in page
    assert page.endswith("<div id='footer'> <p>cmd</p>GeneFuse 0.1.0, at now </div></div></body></html>")
