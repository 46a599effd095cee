"""SURVEY.md §8(f)-4 — what the reference does with the sorted match list: first-fit clustering
into fusion candidates, the break-point refinement, qualification and the text / JSON result
(``FusionMapper::cluster_matches``, src/core/fusion_mapper.rs:399-486 and :544-556;
``FusionResult``, src/core/fusion_result.rs:24-511 and :761-798; ``ReadMatch::print``,
src/core/read_match.rs:153-186; ``JsonReporter::run``, src/core/json_reporter.rs:34-123; ``HtmlReporter::run``,
src/core/html_reporter.rs:195-364 with the protein diagram of fusion_result.rs:462-759).

Host logic, as the reference keeps it on the CPU; the only compute is the edit distance, which is
``gf_edit_distance`` of libgfmatch.so.  That is one library call per comparison, filter and distance,
and ``support`` scans every match of every cluster: fine for the handful of matches of a small run, not
for the 10^5 of a full batch or the thousands of reads a deep panel puts on one junction.  For those,
``report_tail.py`` does the same steps in bulk (libgfreport.so); ``cluster_with`` below is the one body
both share.  Where the
reference would panic (``subchars`` beyond a string's end) this raises ``IndexError``.
``report_html`` writes the HTML report: its ``<body>`` is the reference's byte for byte, the ``<head>`` (script and
style sheet) is this project's own.  The hidden rows of the supporting reads show ``ReadMatch.m_original_reads``, which
the scans attach on request (``originals=True``, scan.py).
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import List, Optional, Sequence

import numpy as np

from .fusion_mapper import ReadMatch, edit_distance, reverse_complement
from .indexer import Fusion, Gene, GenePos


@dataclass
class Settings:
    """src/aux/global_settings.rs:17-24 (defaults)."""
    unique_requirement: int = 2
    deletion_threshold: int = 50
    output_deletions: bool = False
    output_untranslated: bool = False


def _take(s: bytes, skip: int, n: int) -> bytes:
    """``s.chars().skip(skip as usize).take(n as usize)``: a negative i32 cast to usize is huge."""
    if skip < 0:
        return b""
    return s[skip:] if n < 0 else s[skip:skip + n]


def _subchars(s: bytes, pos: int, n: int) -> bytes:
    """utils/mod.rs:36-45: ``self.get(pos..pos+n).unwrap()`` — out of range panics."""
    if pos < 0 or n < 0 or pos + n > len(s):
        raise IndexError("subchars(%d, %d) of a string of %d" % (pos, n, len(s)))
    return s[pos:pos + n]


def dis_connected_count(s: bytes) -> int:
    """utils/mod.rs:48-56."""
    if len(s) == 0:
        raise IndexError("dis_connected_count of an empty string")
    return sum(1 for i in range(len(s) - 1) if s[i] != s[i + 1])


def get_ref_seq(ref: bytes, start: int, end: int) -> bytes:
    """fusion_result.rs:770-798: both ends on one strand and inside the gene, else ""."""
    if (start >= 0 and end <= 0) or (start <= 0 and end >= 0):
        return b""
    if abs(start) >= len(ref) or abs(end) >= len(ref):
        return b""
    n = abs(end - start) + 1
    if start < 0:
        return reverse_complement(ref[-end:-end + n])
    return ref[start:start + n]


def _trunc_div(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


@dataclass
class FusionResult:
    """fusion_result.rs:24-58."""
    m_left_gp: GenePos = GenePos(0, 0)
    m_right_gp: GenePos = GenePos(0, 0)
    m_matches: List[ReadMatch] = field(default_factory=list)
    m_unique: int = 0
    m_title: str = ""
    m_left_ref: bytes = b""
    m_right_ref: bytes = b""
    m_left_ref_ext: bytes = b""
    m_right_ref_ext: bytes = b""
    m_left_pos: str = ""
    m_right_pos: str = ""
    m_left_gene: Gene = field(default_factory=Gene)
    m_right_gene: Gene = field(default_factory=Gene)
    m_left_is_exon: bool = False
    m_right_is_exon: bool = False
    m_left_exon_or_intron_id: int = -1
    m_right_exon_or_intron_id: int = -1

    # -- clustering ------------------------------------------------------------------------
    @staticmethod
    def support_same(m1: ReadMatch, m2: ReadMatch) -> bool:  # :426-445
        return (abs(m1.m_left_gp.position - m2.m_left_gp.position) <= 3 and
                abs(m1.m_right_gp.position - m2.m_right_gp.position) <= 3 and
                m1.m_left_gp.contig == m2.m_left_gp.contig and m1.m_right_gp.contig == m2.m_right_gp.contig)

    def support(self, m: ReadMatch) -> bool:  # :416-424
        return any(self.support_same(m, x) for x in self.m_matches)

    def add_match(self, m: ReadMatch) -> None:  # :412-414
        self.m_matches.append(m)

    # -- the fusion point -------------------------------------------------------------------
    def calc_fusion_point(self) -> None:  # :60-86
        if not self.m_matches:
            return
        lt = rt = 0
        for m in self.m_matches:
            if m.m_gap == 0:  # an exact junction wins
                self.m_left_gp, self.m_right_gp = m.m_left_gp, m.m_right_gp
                return
            lt += m.m_left_gp.position
            rt += m.m_right_gp.position
        n = len(self.m_matches)
        self.m_left_gp = GenePos(self.m_matches[0].m_left_gp.contig, _trunc_div(lt, n))
        self.m_right_gp = GenePos(self.m_matches[0].m_right_gp.contig, _trunc_div(rt, n))

    def make_reference(self, ref_l: bytes, ref_r: bytes) -> None:  # :242-297
        longest_left = longest_right = 0
        for m in self.m_matches:
            longest_left = max(longest_left, m.m_read_break + 1)
            longest_right = max(longest_right, len(m.m_read) - (m.m_read_break + 1))
        lp, rp = self.m_left_gp.position, self.m_right_gp.position
        self.m_left_ref = get_ref_seq(ref_l, lp - longest_left + 1, lp)
        self.m_right_ref = get_ref_seq(ref_r, rp, rp + longest_right - 1)
        self.m_left_ref_ext = get_ref_seq(ref_l, lp, lp + longest_right - 1)
        self.m_right_ref_ext = get_ref_seq(ref_r, rp - longest_left + 1, rp)

    def calc_ed(self, m: ReadMatch, shift: int):  # :326-410 -> (total, left_ed, right_ed)
        seq = m.m_read
        left_len = m.m_read_break + shift + 1
        right_len = len(seq) - left_len
        left_seq = _take(seq, 0, left_len)
        right_seq = _take(seq, left_len, right_len)
        # the 20 bases either side of the break decide the shift ...
        lc = min(len(left_seq), len(self.m_left_ref), 20)
        rc = min(len(right_seq), len(self.m_right_ref), 20)
        total = (edit_distance(left_seq[len(left_seq) - lc:], self.m_left_ref[len(self.m_left_ref) - lc:]) +
                 edit_distance(right_seq[:rc], self.m_right_ref[:rc]))
        # ... the whole overlap gives the distances that are reported
        lc = min(left_len, len(self.m_left_ref))
        rc = min(right_len, len(self.m_right_ref))
        left_ed = edit_distance(_take(left_seq, len(left_seq) - lc, lc),
                                _take(self.m_left_ref, len(self.m_left_ref) - lc, lc))
        right_ed = edit_distance(_take(right_seq, 0, rc), _take(self.m_right_ref, 0, rc))
        return total, left_ed, right_ed

    def best_shift(self, m: ReadMatch):  # :299-324 for one match -> (shift, left distance, right distance)
        smallest, shift = 0xFFFF, 0
        ld, rd = m.m_left_distance, m.m_right_distance
        for s in range(-3, 4):
            ed, l_ed, r_ed = self.calc_ed(m, s)
            if ed < smallest:
                smallest, shift, ld, rd = ed, s, l_ed, r_ed
        return shift, ld, rd

    @staticmethod
    def shifted(m: ReadMatch, shift: int, ld: int, rd: int) -> ReadMatch:
        return replace(m, m_read_break=m.m_read_break + shift,
                       m_left_gp=GenePos(m.m_left_gp.contig, m.m_left_gp.position + shift),
                       m_right_gp=GenePos(m.m_right_gp.contig, m.m_right_gp.position + shift),
                       m_left_distance=ld, m_right_distance=rd)

    def adjust_fusion_break(self) -> None:  # :299-324
        self.m_matches = [self.shifted(m, *self.best_shift(m)) for m in self.m_matches]

    def calc_unique(self) -> None:  # :88-105 (the list is sorted: compare neighbours)
        self.m_unique = 1
        for prev, m in zip(self.m_matches, self.m_matches[1:]):
            if m.m_read_break != prev.m_read_break or len(m.m_read) != len(prev.m_read):
                self.m_unique += 1

    # -- what it is ---------------------------------------------------------------------------
    def is_deletion(self) -> bool:  # :107-118
        l, r = self.m_left_gp, self.m_right_gp
        return l.contig == r.contig and ((l.position > 0 and r.position > 0) or (l.position < 0 and r.position < 0))

    def is_left_protein_forward(self) -> bool:  # :446-452
        p = self.m_left_gp.position
        return p < 0 if self.m_left_gene.is_reversed() else p > 0

    def is_right_protein_forward(self) -> bool:  # :454-460
        p = self.m_right_gp.position
        return p < 0 if self.m_right_gene.is_reversed() else p > 0

    def update_info(self, fusions: Sequence[Fusion]) -> None:  # :196-240
        self.m_left_gene = fusions[self.m_left_gp.contig].m_gene
        self.m_right_gene = fusions[self.m_right_gp.contig].m_gene
        self.m_left_pos = self.m_left_gene.pos2str(self.m_left_gp.position)
        self.m_right_pos = self.m_right_gene.pos2str(self.m_right_gp.position)
        self.m_title = "%s%s___%s  (total: %d, unique:%d)" % (
            "Deletion: " if self.is_deletion() else "Fusion: ", self.m_left_pos, self.m_right_pos,
            len(self.m_matches), self.m_unique)
        e, k = self.m_left_gene.get_exon_intron(self.m_left_gp.position)
        if e is not None:  # (the reference's out-parameters stay as they were otherwise)
            self.m_left_is_exon, self.m_left_exon_or_intron_id = e, k
        e, k = self.m_right_gene.get_exon_intron(self.m_right_gp.position)
        if e is not None:
            self.m_right_is_exon, self.m_right_exon_or_intron_id = e, k

    @staticmethod
    def can_be_matched(s1: bytes, s2: bytes) -> bool:  # :131-161
        n = len(s1)
        for offset in range(-6, 7):
            start1, start2 = max(offset, 0), max(-offset, 0)
            cmplen = n - abs(offset)
            if start1 >= len(s1) or start2 >= len(s2):
                return True
            ed = edit_distance(_subchars(s1, start1, cmplen), _subchars(s2, start2, cmplen))
            if ed <= _trunc_div(cmplen, 10):
                return True
        return False

    def can_be_mapped(self) -> bool:  # :120-129: the two sides continue each other's gene
        return (self.can_be_matched(self.m_left_ref_ext, self.m_right_ref) or
                self.can_be_matched(self.m_left_ref, self.m_right_ref_ext))

    def is_qualified(self, settings: Settings) -> bool:  # :163-194
        if self.m_unique < settings.unique_requirement:
            return False
        if self.can_be_mapped():
            return False
        if len(self.m_left_ref) <= 30 or len(self.m_right_ref) <= 30:
            return False
        if dis_connected_count(_subchars(self.m_left_ref, len(self.m_left_ref) - 10, 10)) <= 2:
            return False
        if dis_connected_count(_subchars(self.m_right_ref, 0, 10)) <= 2:
            return False
        return True

    # -- output -------------------------------------------------------------------------------
    def text(self) -> str:
        """``FusionResult::print`` (:761-767) over ``ReadMatch::print`` (read_match.rs:153-186)."""
        out = ["\n#%s\n" % self.m_title]
        for i, m in enumerate(self.m_matches):
            name = _subchars(m.m_name, 1, len(m.m_name) - 1).decode("latin-1")
            b = m.m_read_break + 1
            out.append(">%d, break:%d, diff:(%d %d), read direction: %s, name: %s\n%s %s\n" % (
                i + 1, b, m.m_left_distance, m.m_right_distance,
                "reversed complement" if m.m_reversed else "original direction", name,
                _subchars(m.m_read, 0, b).decode("latin-1"),
                _subchars(m.m_read, b, len(m.m_read) - b).decode("latin-1")))
        return "".join(out)


def match_group(m: ReadMatch, n_fusions: int) -> int:
    """FusionMapper::add_match (fusion_mapper.rs:253-275): the list a match is kept in."""
    return n_fusions * m.m_right_gp.contig + m.m_left_gp.contig


def first_fit_clusters(groups: Sequence[Sequence[ReadMatch]]) -> List[FusionResult]:
    """The first fit of fusion_mapper.rs:399-420: every match joins the first cluster of its group that supports it,
    or founds one.  The clusters of all groups, in the order they were made."""
    out: List[FusionResult] = []
    for fm in groups:
        frs: List[FusionResult] = []
        for rm in fm:
            for fr in frs:
                if fr.support(rm):
                    fr.add_match(rm)
                    break
            else:
                fr = FusionResult()
                fr.add_match(rm)
                frs.append(fr)
        out += frs
    return out


def adjust_clusters(frs: Sequence[FusionResult]) -> None:
    for fr in frs:
        fr.adjust_fusion_break()


def cluster_with(groups: Sequence[Sequence[ReadMatch]], fusions: Sequence[Fusion], fusion_seq: Sequence[str],
                 settings: Optional[Settings], first_fit, adjust) -> List[FusionResult]:
    """fusion_mapper.rs:399-486 + sort_fusion_results (:544-556), with the two steps that have a bulk form handed in:
    ``first_fit(groups)`` gives the clusters of all groups in the order they are made, ``adjust(clusters)`` refines the
    breaks of all their matches.  The clusters do not depend on one another, so running a step for all of them before
    the next step gives what the reference's cluster-by-cluster loop gives."""
    settings = settings or Settings()
    frs = first_fit(groups)
    for fr in frs:
        fr.calc_fusion_point()
        fr.make_reference(fusion_seq[fr.m_left_gp.contig].encode("latin-1"),
                          fusion_seq[fr.m_right_gp.contig].encode("latin-1"))
    adjust(frs)
    results: List[FusionResult] = []
    for fr in frs:
        fr.calc_unique()
        fr.update_info(fusions)
        if not fr.is_qualified(settings):
            continue
        if not settings.output_deletions and fr.is_deletion():
            continue
        if fr.is_left_protein_forward() != fr.is_right_protein_forward() and not settings.output_untranslated:
            continue
        results.append(fr)
    results.sort(key=lambda fr: (-fr.m_unique, -len(fr.m_matches)))  # stable, like sort_by
    return results


def cluster_matches(groups: Sequence[Sequence[ReadMatch]], fusions: Sequence[Fusion], fusion_seq: Sequence[str],
                    settings: Optional[Settings] = None) -> List[FusionResult]:
    """fusion_mapper.rs:399-486 + sort_fusion_results (:544-556).  ``groups`` = the reference's
    ``fusion_matches``: one sorted list per (right, left) gene pair, in ``match_group`` order.
    ``fusion_seq`` = ``Indexer.m_fusion_seq``."""
    return cluster_with(groups, fusions, fusion_seq, settings, first_fit_clusters, adjust_clusters)


def group_and_sort(matches: Sequence[ReadMatch], n_fusions: int, sort=None) -> List[List[ReadMatch]]:
    """The reference's ``fusion_matches`` after ``sort_matches`` (fusion_mapper.rs:379-384): the
    non-empty lists only, in index order (empty ones produce nothing in ``cluster_matches``).  ``sort``: what sorts a
    list, ``FusionMapper.sort_matches`` unless given."""
    from .fusion_mapper import FusionMapper
    sort = sort or FusionMapper.sort_matches
    by: dict = {}
    for m in matches:
        by.setdefault(match_group(m, n_fusions), []).append(m)
    return [sort(by[k]) for k in sorted(by)]


def report_text(results: Sequence[FusionResult]) -> str:
    return "".join(fr.text() for fr in results)


def report_json(results: Sequence[FusionResult], command: str, version: str, time: str,
                settings: Optional[Settings] = None) -> str:
    """The bytes ``JsonReporter::run`` writes (json_reporter.rs:34-123), tabs and trailing blanks
    included; ``time`` is whatever the caller wants on the reference's ``Local::now()`` line."""
    settings = settings or Settings()
    f: List[str] = ["{\n", "\t\"command\":\"%s\",\n" % command, "\t\"version\":\"%s\",\n" % version,
                    "\t\"time\":\"%s\",\n" % time, "\t\"fusions\":{"]
    first = True
    for fr in results:
        if _skipped(fr, settings):
            continue
        f.append("\n" if first else ",\n")
        first = False
        f.append("\t\t\"%s\":{\n" % fr.m_title)
        for side, gene, gp, ref, ext, pos, is_exon, eid, fwd in (
                ("left", fr.m_left_gene, fr.m_left_gp, fr.m_left_ref, fr.m_left_ref_ext, fr.m_left_pos,
                 fr.m_left_is_exon, fr.m_left_exon_or_intron_id, fr.is_left_protein_forward()),
                ("right", fr.m_right_gene, fr.m_right_gp, fr.m_right_ref, fr.m_right_ref_ext, fr.m_right_pos,
                 fr.m_right_is_exon, fr.m_right_exon_or_intron_id, fr.is_right_protein_forward())):
            f.append("\t\t\t\"%s\":{\n" % side)
            f.append("\t\t\t\t\"gene_name\":\"%s\",\n" % gene.m_name)
            f.append("\t\t\t\t\"gene_chr\":\"%s\",\n" % gene.m_chr)
            f.append("\t\t\t\t\"position\":%d,\n" % gene.gene_pos_2_chr_pos(gp.position))
            f.append("\t\t\t\t\"reference\":\"%s\",\n" % ref.decode("latin-1"))
            f.append("\t\t\t\t\"ref_ext\":\"%s\",\n" % ext.decode("latin-1"))
            f.append("\t\t\t\t\"pos_str\":\"%s\",\n" % pos)
            f.append("\t\t\t\t\"exon_or_intron\":\"%s\",\n" % ("exon" if is_exon else "intron"))
            f.append("\t\t\t\t\"exon_or_intron_id\":%d,\n" % eid)
            f.append("\t\t\t\t\"strand\":\"%s\"\n" % ("forward" if fwd else "reversed"))
            f.append("\t\t\t}, \n")
        f.append("\t\t\t\"unique\":%d,\n" % fr.m_unique)
        f.append("\t\t\t\"reads\":[\n")
        for k, m in enumerate(fr.m_matches):
            f.append("\t\t\t\t{\n")
            f.append("\t\t\t\t\t\"break\":%d,\n" % m.m_read_break)
            f.append("\t\t\t\t\t\"strand\":\"%s\",\n" % ("reversed" if m.m_reversed else "forward"))
            f.append("\t\t\t\t\t\"seq\":\"%s\",\n" % m.m_read.decode("latin-1"))
            f.append("\t\t\t\t\t\"qual\":\"%s\"\n" % m.m_quality.decode("latin-1"))
            f.append("\t\t\t\t}" + ("," if k != len(fr.m_matches) - 1 else "") + "\n")
        f.append("\t\t\t]\n")
        f.append("\t\t}")
    f.append("\n\t}\n}\n\n")
    return "".join(f)


# ---- the HTML report ------------------------------------------------------------------------------------------------

_F32 = np.float32


def _skipped(fr: FusionResult, settings: Settings) -> bool:
    """What the reporters leave out (html_reporter.rs:263-270, json_reporter.rs): deletions and direction conflicts,
    unless the settings ask for them."""
    if not settings.output_deletions and fr.is_deletion():
        return True
    return fr.is_left_protein_forward() != fr.is_right_protein_forward() and not settings.output_untranslated


def _text(b: bytes) -> str:
    """Bytes of the input files as text that ``write_report`` turns back into the same bytes."""
    return b.decode("utf-8", "surrogateescape")


def quality_color(q: int) -> str:
    """read.rs:275-297: the colour of a base by its quality character (a byte value)."""
    if q >= ord("I"):    # >= Q40
        return "#78C6B9"
    if q >= ord("?"):    # Q30 ~ Q39
        return "#33BBE2"
    if q >= ord("5"):    # Q20 ~ Q29
        return "#666666"
    if q >= ord("0"):    # Q15 ~ Q19
        return "#E99E5B"
    return "#FF0000"


def _html_seq_with_qual(m: ReadMatch, start: int, length: int) -> str:
    """read.rs:199-213; a quality string shorter than the read panics there."""
    out = []
    for i in range(max(start, 0), min(start + length, len(m.m_read))):
        if i >= len(m.m_quality):
            raise IndexError("base %d of a read with %d qualities" % (i, len(m.m_quality)))
        out.append("<a title='%s'><font color='%s'>%s</font></a>" % (
            _text(m.m_quality[i:i + 1]), quality_color(m.m_quality[i]), _text(m.m_read[i:i + 1])))
    return "".join(out)


def html_read_row(m: ReadMatch, number: int) -> str:
    """The cells of a supporting read's row, from ``<td>`` to the last ``</td>`` (html_reporter.rs:338-351,
    read_match.rs:92-113, read.rs:127-165 with the one break): ``number`` is the row's, from 1."""
    b = m.m_read_break + 1
    out = ["<td><a title='%s'>%04d%s</a></span></td><td>%d|%d</td>" % (
        _text(m.m_name), number, "\u2190" if m.m_reversed else "\u2192", m.m_left_distance, m.m_right_distance)]
    out.append("<td class='alignright'>%s</td>" % _html_seq_with_qual(m, 0, b))
    if b > 0:
        out.append("<td class='alignleft'>%s</td>" % _html_seq_with_qual(m, b, len(m.m_read) - b))
    return "".join(out)


def html_original_reads(m: ReadMatch) -> str:
    """read_match.rs:115-120 over read.rs:263-272: the four lines of every original record, a newline after each."""
    return "".join(_text(line) + "\n" for rec in m.m_original_reads for line in rec)


def _round_away(x) -> float:
    """f32::round: half away from zero (Python's ``round`` goes to even)."""
    x = float(x)
    if x != x or x in (float("inf"), float("-inf")):
        return x
    r = float(int(abs(x) + 0.5))
    return r if x >= 0 else -r


def _as_i32(x) -> int:
    """Rust's ``as i32`` of a float: towards zero, saturating, NaN is 0."""
    x = float(x)
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


def exon_intron_numbers(fr: FusionResult):
    """fusion_result.rs:462-512 in f32: (left exons, left introns, right exons, right introns) that the diagram draws;
    halves stand for the exon or intron the break lies in.  A gene without exons underflows ``total_exon - 1`` there."""
    out = []
    for gene, is_exon, eid, counts_up in (
            (fr.m_left_gene, fr.m_left_is_exon, fr.m_left_exon_or_intron_id, fr.is_left_protein_forward()),
            (fr.m_right_gene, fr.m_right_is_exon, fr.m_right_exon_or_intron_id, not fr.is_right_protein_forward())):
        total_exon = len(gene.m_exons)
        if total_exon == 0:
            raise IndexError("gene %s has no exons" % gene.m_name)
        total_intron = total_exon - 1
        if counts_up:    # the part of the gene in front of the break, counted from exon 1
            exon = _F32(eid) - _F32(0.5) if is_exon else _F32(eid)
            intron = _F32(eid) - _F32(1.0) if is_exon else _F32(eid) - _F32(0.5)
        else:            # the part behind it, counted from the last exon
            exon = _F32(total_exon - eid) + _F32(0.5) if is_exon else _F32(total_exon - eid)
            intron = _F32(total_intron - eid) + (_F32(1.0) if is_exon else _F32(0.5))
        out += [exon, intron]
    return tuple(out)


def _exon_intron_td(is_exon: bool, forward: bool, number: int, percent, style: str) -> str:  # :727-759
    width = _as_i32(percent)
    if width <= 0:
        width = 1
    return "<td class='%s' width='%d%%'>%s</td>" % (
        style, width, "E%d" % number if is_exon else ("\u2192" if forward else "\u2190"))


def html_protein(fr: FusionResult) -> str:
    """``print_fusion_protein_html`` (fusion_result.rs:514-725): the two genes' exons and introns up to and from the
    break, as nested tables.  The ``protein_right`` cell carries the left percentage, as in the reference."""
    le, li, re_, ri = exon_intron_numbers(fr)
    with np.errstate(all="ignore"):
        left_size, right_size = le + li, re_ + ri
        left_percent = _as_i32(_round_away(left_size * _F32(100.0) / (left_size + right_size)))
        right_percent = 100 - left_percent
        left_percent, right_percent = left_percent or 1, right_percent or 1
        out = ["<table width='100%' class='protein_table'>\n<tr>",
               "<td width='%d%%'>%s</td><td width='%d%%'>%s</td></tr><tr>" % (
                   left_percent, fr.m_left_gene.m_name, right_percent, fr.m_right_gene.m_name),
               "<td class='protein_left' width='%d%%'>" % left_percent]
        # -- the left gene (:579-648): whole steps, the last one a half
        step_percent = _F32(100.0) / (le + li)
        half = step_percent * _F32(0.5)
        forward = fr.is_left_protein_forward()
        exon, intron, step = 1, 1, 1
        if not forward:
            exon = len(fr.m_left_gene.m_exons)
            intron, step = exon - 1, -1
        out.append("<table width='100%' class='protein_table'>\n<tr>")
        done_e = done_i = _F32(0.0)
        while done_e < le or done_i < li:
            if done_e < le:
                out.append(_exon_intron_td(True, forward, exon, half if done_e + _F32(1.0) > le else step_percent,
                                           "exon_left"))
                done_e += _F32(1.0)
                exon += step
            if done_i < li:
                out.append(_exon_intron_td(False, forward, intron, half if done_i + _F32(1.0) > li else step_percent,
                                           "intron_left"))
                done_i += _F32(1.0)
                intron += step
        out.append("</tr></table></td><td class='protein_right' width='%d%%'>" % left_percent)
        # -- the right gene (:650-725): the first step is the half
        step_percent = _F32(100.0) / (re_ + ri)
        half = step_percent * _F32(0.5)
        forward = fr.is_right_protein_forward()
        exon = intron = fr.m_right_exon_or_intron_id
        step = 1 if forward else -1
        out.append("<table width='100%' class='protein_table'>\n<tr>")
        done_e = done_i = _F32(0.0)
        if not fr.m_right_is_exon:
            out.append(_exon_intron_td(False, forward, intron, half, "intron_right"))
            done_i += _F32(0.5)
            intron += step
            if forward:
                exon += step
        while done_e < re_ or done_i < ri:
            if done_e < re_:
                first_half = fr.m_right_is_exon and done_e == 0.0
                out.append(_exon_intron_td(True, forward, exon, half if first_half else step_percent, "exon_right"))
                done_e += _F32(0.5) if first_half else _F32(1.0)
                exon += step
            if done_i < ri:
                out.append(_exon_intron_td(False, forward, intron, step_percent, "intron_right"))
                done_i += _F32(1.0)
                intron += step
        out.append("</tr></table></td></tr></table>")
    return "".join(out)


def _html_fusion(id_: int, fr: FusionResult) -> str:  # html_reporter.rs:279-364
    conflict = fr.is_left_protein_forward() != fr.is_right_protein_forward()
    lr, lx, rr, rx = (_text(x) for x in (fr.m_left_ref, fr.m_left_ref_ext, fr.m_right_ref, fr.m_right_ref_ext))
    out = ["<div class='fusion_block'><div class='fusion_head'><a name='fusion_id_%d'>%d, %s</a></div>" % (
               id_, id_, fr.m_title),
           "<div class='tips'>Inferred protein%s:</div>" % (
               " (transcription direction conflicts, this fusion may be not transcribed) " if conflict else ""),
           html_protein(fr),
           "<div class='tips'>Supporting reads:</div><table><tr class='header'>",
           "<td class='alignright' colspan='3'>%s = <font color='yellow'>\u2193</font></td>" % fr.m_left_pos,
           "<td class='alignleft'><font color='yellow'>\u2193</font> = %s</td></tr><tr class='header'>" % fr.m_right_pos,
           "<td class='alignright' colspan='3'><a title='%s___%s'>%s</a></td>" % (lr, lx, lr),
           "<td class='alignleft'><a title='%s___%s'>%s</a></td></tr>" % (rx, rr, rr)]
    for k, m in enumerate(fr.m_matches):
        row = id_ * 100000 + k
        out.append("<tr onclick='toggle(%d);'>%s</tr>" % (row, html_read_row(m, k + 1)))
        out.append("<tr id='%d' style='display:none;'><td colspan='6'><xmp>%s</xmp></td></tr>" % (
            row, html_original_reads(m)))
    out.append("</table></div>")
    return "".join(out)


_HTML_HELPER = (
    "<div id='helper'><p>Helpful tips:</p><ul>"
    "<li> Base color indicates quality: <font color='#78C6B9'>extremely high (Q40+)</font>, "
    "<font color='#33BBE2'>high (Q30~Q39) </font>, <font color='#666666'>moderate (Q20~Q29)</font>, "
    "<font color='#E99E5B'>low (Q15~Q19)</font>, <font color='#FF0000'>extremely low (0~Q14).</font> </li>"
    "<li> Move mouse over the base, it will show the quality value</li>"
    "<li> Click on any row, the original read/pair will be displayed</li>"
    "<li> For pair-end sequencing, GeneFuse tries to merge each pair, with overlapped assigned higher qualities </li>"
    "</ul><p>Columns:</p><ul>"
    "<li> col1: is fusion mapped with original read? \u2192 means original read, \u2190 means reverse complement</li>"
    "<li> col2: edit distance (ed) between read and reference sequence (left_part_ed | right_part_ed)</li>"
    "<li> col3: read's left part after fusion break</li>"
    "<li> col4: read's right part after fusion break</li>"
    "</ul></div>")

# This project's own head: the body needs toggle(id) and the class names below, nothing more.
_HTML_SCRIPT = (
    "<script type=\"text/javascript\">\n"
    "function toggle(id) {\n"
    "  var row = document.getElementById(id);\n"
    "  if (row) { row.style.display = (row.style.display === 'table-row') ? 'none' : 'table-row'; }\n"
    "}\n"
    "</script>")
_HTML_STYLE = (
    "<style type=\"text/css\">\n"
    "body { margin: 0; }\n"
    "#container { font-family: Menlo, Consolas, monospace; text-align: center; padding: 4px; }\n"
    "table { border-collapse: collapse; border: 1px solid #888; }\n"
    "td { border: 1px solid #ddd; padding: 0 2px; font-size: 10px; }\n"
    ".alignleft { text-align: left; }\n"
    ".alignright { text-align: right; }\n"
    ".software { font-size: 22px; font-weight: bold; padding: 6px; }\n"
    ".header { background: #111; color: #fff; height: 20px; }\n"
    "#menu { text-align: left; padding: 10px 0; }\n"
    "#menu a { color: #0b5cad; font-size: 17px; text-decoration: none; }\n"
    ".menu_item { text-align: left; padding-top: 4px; }\n"
    ".fusion_head { text-align: left; color: #0b7fd6; padding: 18px 0 4px 0; }\n"
    ".fusion_block { margin-bottom: 8px; }\n"
    ".tips { text-align: left; color: #555; font-size: 10px; padding: 4px; }\n"
    "#helper { text-align: left; color: #666; font-size: 12px; }\n"
    "#footer { text-align: left; color: #666; font-size: 10px; padding: 18px 0 0 8px; }\n"
    ".protein_table { text-align: center; font-size: 8px; }\n"
    ".protein_left, .protein_right { padding: 0; }\n"
    ".exon_left { background: #1f3fbf; color: #fff; border: 0; padding: 0; font-size: 8px; }\n"
    ".exon_right { background: #c22; color: #fff; border: 0; padding: 0; font-size: 8px; }\n"
    ".intron_left { color: #1f3fbf; padding: 0; font-size: 8px; }\n"
    ".intron_right { color: #c22; padding: 0; font-size: 8px; }\n"
    "</style>")


def html_body(results: Sequence[FusionResult], command: str, version: str, time: str,
              settings: Optional[Settings] = None) -> str:
    """``<body>`` through ``</html>`` as ``HtmlReporter::run`` writes it (html_reporter.rs:72-79, :195-364).  The menu
    lists every result, numbered over all of them; the blocks leave deletions and direction conflicts out under the
    settings and number themselves."""
    settings = settings or Settings()
    out = ["<body><div id='container'><div class='software'> <a href='https://github.com/OpenGene/GeneFuse' "
           "style='text-decoration:none;' target='_blank'>GeneFuse</a> <font size='-1'>%s</font></div>" % version,
           _HTML_HELPER,
           "<div id='menu'><p>Found %d fusion%s:</p><ul>" % (len(results), "s" if len(results) > 1 else "")]
    for k, fr in enumerate(results):
        out.append("<li class='menu_item'><a href='#fusion_id_%d'> %d, %s</a></li>" % (k + 1, k + 1, fr.m_title))
    out.append("</ul></div>")
    id_ = 0
    for fr in results:
        if _skipped(fr, settings):
            continue
        id_ += 1
        out.append(_html_fusion(id_, fr))
    out.append("<div id='footer'> <p>%s</p>GeneFuse %s, at %s </div></div></body></html>" % (command, version, time))
    return "".join(out)


def report_html(results: Sequence[FusionResult], command: str, version: str, time: str,
                settings: Optional[Settings] = None) -> str:
    """The HTML report, the counterpart of ``report_json``: ``time`` is whatever the caller wants where the reference
    writes ``Local::now()``.  Byte parity with ``HtmlReporter::run`` is claimed for ``<body>`` .. ``</body>`` only
    (``html_body``): the ``<title>`` follows the reference's pattern, the script and the style sheet are this
    project's own.  Bytes of the input files (names, bases, qualities, original records) pass through unescaped, as in
    the reference; ``write_report`` writes the text as those bytes."""
    return ("<html><head><meta http-equiv=\"content-type\" content=\"text/html;charset=utf-8\" />"
            "<title>GeneFuse %s, at %s</title>%s%s</head>" % (version, time, _HTML_SCRIPT, _HTML_STYLE) +
            html_body(results, command, version, time, settings))


def write_report(path: str, text: str) -> None:
    """A report text to a file, as UTF-8 with the input files' own bytes restored."""
    with open(path, "w", encoding="utf-8", errors="surrogateescape", newline="") as f:
        f.write(text)
