"""The host text layer -- jplace writer and reader, newick and model-descriptor parsers, FASTA / bfast / FASTQ readers --
run in a stand-alone driver (tests/host_driver/host_text_driver.cpp, built by host_driver_util) under the address and
undefined-behaviour sanitizers and again with the product's -O2.  CPU only: the driver links no device library.

Every case runs on both builds and asserts exit status 0, nothing on stderr (so: no sanitizer report) and the expected
line.  The writer is held against an independent restatement in Python ('%.*f' and the layout of jplace_chunk_text /
write_jplace_text), compared with == on the whole file; readers against plain Python parsers; the tree's likelihood
against the oracle.

Not covered on purpose: read names are written into "n" raw, without JSON escaping, as the reference writes them
(src/io/jplace_util.cpp:83-90); the names used here need none."""
import json
import math
import os
import re
import struct

import pytest

import host_driver_util as hd

VARIANTS = hd.VARIANTS

# ---------------------------------------------------------------------------------------------------------------------
# writer
# ---------------------------------------------------------------------------------------------------------------------
PRECISIONS = (0, 1, 10, 18, 19, 40, 66, 70, 250, 340, 1100)
VALUES = (-4620.363834217626, 0.0, -0.0, 0.5, 0.125, 5e-324, 1e-300, 1e22, 1.7976931348623157e308,
          math.inf, -math.inf, math.nan)
FINITE = VALUES[:9]
# Jplace_Fields bit -> (indices into a row's 15 values, names), in the order the writer emits them
EXTRAS = ((1, (4,), ("rell_support",)), (4, (5, 6), ("elw", "p_sh")), (8, (7,), ("p_au",)),
          (16, (8, 9, 10), ("p_kh", "p_wkh", "p_wsh")), (2, (11, 12), ("marginal_like", "post_prob")),
          (32, (13, 14), ("exp_dist", "edpl")))
NEWICK = "((a:0.1{0},b:0.2{1}):0.05{2},c:0.3{3},d:0.4{4});"
INVOCATION = "epa-ng-amd --tree t.nwk --ref-msa r.fasta --query q.fasta"
# a mapper whose root edge (5) splits at distal length 0.25 and whose edge 9 maps to the largest edge id
MAPPER = dict(map=[0, 11, 12, 13, 14, 15, 16, 17, 18, 4294967295, 20], root=5, prox_edge=7, dist_edge=3, prox_len=0.75,
              dist_len=0.25)
ROWS = (1, 2, 7)


def value_columns(extra):
    cols = [0, 1, 2, 3]   # likelihood, like_weight_ratio, distal_length, pendant_length
    for bit, idx, _ in EXTRAS:
        if extra & bit:
            cols += idx
    return cols


def field_names(extra):
    names = ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "pendant_length"]
    for bit, _, n in EXTRAS:
        if extra & bit:
            names += n
    return names


def in_rtree(mapper, edge, distal):
    """Rtree_Mapper::in_rtree restated"""
    if edge == mapper["root"]:
        if distal > mapper["dist_len"]:
            return mapper["prox_edge"], mapper["prox_len"] - (distal - mapper["dist_len"])
        return mapper["dist_edge"], distal
    return mapper["map"][edge], distal


def expected_rows(case):
    """per chunk, per object: (name, [(edge, [values in written order])]) after the mapper"""
    cols = value_columns(case["extra"])
    out = []
    for chunk in case["chunks"]:
        objs = []
        for name, rows in chunk:
            wr = []
            for edge, v in rows:
                v = list(v)
                if case["mapper"]:
                    edge, v[2] = in_rtree(case["mapper"], edge, v[2])
                wr.append((edge, [v[c] for c in cols]))
            objs.append((name, wr))
        out.append(objs)
    return out


def expected_document(case):
    p = case["precision"]
    texts = []
    for objs in expected_rows(case):
        t = ""
        for i, (name, rows) in enumerate(objs):
            t += "    {\"p\": [\n"
            for j, (edge, vals) in enumerate(rows):
                t += "      [" + str(edge) + "".join(", " + "%.*f" % (p, v) for v in vals) + "]"
                t += (",\n" if j + 1 < len(rows) else "\n")
            t += "      ],\n    \"n\": [\"" + name + "\"]\n    }" + ("," if i + 1 < len(objs) else "") + "\n"
        texts.append(t)
    return ("{\n  \"tree\": \"" + NEWICK + "\",\n  \"placements\": \n  [\n" + ",\n".join(t for t in texts if t) +
            "  ],\n  \"metadata\": {\"invocation\": \"" + INVOCATION + "\"},\n  \"version\": 3,\n  \"fields\": [" +
            ", ".join("\"" + n + "\"" for n in field_names(case["extra"])) + "]\n}\n")


def make_case(precision, extra, threads, mapped, objects=(1, 2, 7), values=VALUES, shift=0):
    """chunks of 1, 2 and 7 objects whose objects have 1, 2 and 7 rows in turn; row g of the case carries
    values[(g + f + shift) % len] in field f, so every value stands in every field once the case has len(values) rows"""
    edges = (0, 9, 5) if mapped else (0, 9, 4294967295)
    chunks, g = [], shift
    for ci, nobj in enumerate(objects):
        chunk = []
        for o in range(nobj):
            rows = []
            for _ in range(ROWS[(o + ci + shift) % 3]):
                rows.append((edges[g % 3], [values[(g + f) % len(values)] for f in range(15)]))
                g += 1
            chunk.append(("read_%d_%d" % (ci, o), rows))
        chunks.append(chunk)
    assert g - shift >= len(values) or len(objects) == 1
    return dict(precision=precision, extra=extra, threads=threads, mapper=MAPPER if mapped else None, chunks=chunks)


def spec_text(cases):
    w = []
    for c in cases:
        w.append("case %d %d %d %s %s %d" % (c["precision"], c["extra"], c["threads"], NEWICK.encode().hex(),
                                             INVOCATION.encode().hex(), len(c["chunks"])))
        m = c["mapper"]
        if m:
            w.append("mapper %d %s %d %d %d %s %s" % (len(m["map"]), " ".join(map(str, m["map"])), m["root"], m["prox_edge"],
                                                       m["dist_edge"], float(m["prox_len"]).hex(), float(m["dist_len"]).hex()))
        else:
            w.append("mapper 0")
        for chunk in c["chunks"]:
            w.append("chunk %d" % len(chunk))
            for name, rows in chunk:
                w.append("pq %s %d" % (name.encode().hex(), len(rows)))
                for edge, v in rows:
                    w.append("row %d %s" % (edge, " ".join(float(x).hex() for x in v)))
    return "\n".join(w) + "\n"


def write_cases(variant, tmp_path, cases):
    """the driver's documents of `cases`, one text each"""
    spec = tmp_path / "spec.txt"
    spec.write_text(spec_text(cases))
    outdir = tmp_path / ("out_" + variant)
    outdir.mkdir(exist_ok=True)
    lines = hd.run(variant, ["writer", spec, outdir])
    assert len(lines) == len(cases)
    docs = []
    for i, line in enumerate(lines):
        assert line.startswith("ok %d " % i), line
        docs.append((outdir / ("%d.jplace" % i)).read_bytes().decode())
    return docs


def first_difference(a, b):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return "lengths %d / %d, first difference at byte %d: %r / %r" % (len(a), len(b), n, a[max(0, n - 40):n + 40], b[max(0, n - 40):n + 40])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_writer_equals_its_restatement_for_all_field_sets(variant, precision, tmp_path):
    """all 64 sets of the six optional field groups at one precision; thread counts 1, 2, 5 and mapper on / off take
    turns over the cases (the cross of those is the next test).  The 1-object chunk leaves 1 or 4 threads of a team of
    2 or 5 with an empty range."""
    cases = [make_case(precision, extra, (1, 2, 5)[extra % 3], (extra // 3) % 2 == 1, shift=extra) for extra in range(64)]
    for case, got in zip(cases, write_cases(variant, tmp_path, cases)):
        want = expected_document(case)
        assert got == want, (case["extra"], case["threads"], bool(case["mapper"]), first_difference(got, want))


@pytest.mark.parametrize("variant", VARIANTS)
def test_writer_threads_mapper_and_object_counts(variant, tmp_path):
    """threads 1, 2, 5 x mapper on / off x chunks of 1, 2, 7 objects alone and together, with no extra field and with
    all of them, at every precision"""
    cases = []
    for precision in PRECISIONS:
        for extra in (0, 63):
            for threads in (1, 2, 5):
                for mapped in (False, True):
                    for objects in ((1,), (2,), (7,), (1, 2, 7)):
                        if precision > 100 and objects != (1, 2, 7):
                            continue   # the long rows once per thread count: they take the same path for any object count
                        cases.append(make_case(precision, extra, threads, mapped, objects=objects))
    for case, got in zip(cases, write_cases(variant, tmp_path, cases)):
        want = expected_document(case)
        assert got == want, (case["precision"], case["extra"], case["threads"], bool(case["mapper"]), first_difference(got, want))


@pytest.mark.parametrize("variant", VARIANTS)
def test_writer_empty_chunks_and_objects_without_rows(variant, tmp_path):
    """chunks without objects are skipped by write_jplace_text; an object without rows keeps its frame"""
    case = make_case(10, 63, 5, False)
    case["chunks"] = [[], case["chunks"][1], [], [("lonely", [])], []]
    none = dict(precision=10, extra=0, threads=2, mapper=None, chunks=[[], []])
    docs = write_cases(variant, tmp_path, [case, none])
    assert docs[0] == expected_document(case) and docs[1] == expected_document(none)
    assert json.loads(docs[1])["placements"] == []


@pytest.mark.parametrize("variant", VARIANTS)
def test_round_trip_through_json_and_read_jplace(variant, tmp_path):
    """finite values written, then parsed by Python's json and by read_jplace: edge, distal and pendant come back as the
    doubles nearest to the written decimal text"""
    cases = [make_case(p, extra, 2, mapped, values=FINITE, shift=s)
             for p in (0, 1, 10, 18, 19, 40, 70, 340) for s, (extra, mapped) in enumerate(((0, False), (63, True), (21, False)))]
    spec = tmp_path / "spec.txt"
    spec.write_text(spec_text(cases))
    outdir = tmp_path / "rt"
    outdir.mkdir()
    assert len(hd.run(variant, ["writer", spec, outdir])) == len(cases)
    files = [outdir / ("%d.jplace" % i) for i in range(len(cases))]
    lines = hd.run(variant, ["readjplace"] + files)
    assert len(lines) == len(cases)
    for case, f, line in zip(cases, files, lines):
        p = case["precision"]
        doc = json.loads(f.read_text(), parse_int=float)   # "-0" (precision 0) is an int to Python's json: the sign would go
        assert doc["fields"] == field_names(case["extra"]) and doc["version"] == 3.0 and doc["tree"] == NEWICK
        want = []   # (name, [(edge, nearest double of distal's text, of pendant's text)])
        for objs in expected_rows(case):
            for name, rows in objs:
                want.append((name, [(e, float("%.*f" % (p, v[2])), float("%.*f" % (p, v[3]))) for e, v in rows]))
        got_json = [(o["n"][0], [(int(r[0]), r[3], r[4]) for r in o["p"]]) for o in doc["placements"]]
        assert all(r[0] == int(r[0]) for o in doc["placements"] for r in o["p"])
        assert repr(got_json) == repr(want)   # repr: -0.0 is not 0.0
        toks = line.split(" ")
        assert toks[0] == "ok" and int(toks[1]) == len(want)
        got = []
        for t in toks[2:]:
            parts = t.split(",")
            got.append((hd.unhex(parts[0]).decode(), [(int(e), float.fromhex(d), float.fromhex(q)) for e, d, q in (x.split(":") for x in parts[1:])]))
        assert repr(got) == repr(want)


# ---------------------------------------------------------------------------------------------------------------------
# reader
# ---------------------------------------------------------------------------------------------------------------------
def read_lines(variant, tmp_path, docs):
    files = []
    for i, d in enumerate(docs):
        f = tmp_path / ("r%s_%d.jplace" % (variant, i))
        f.write_bytes(d if isinstance(d, bytes) else d.encode())
        files.append(f)
    lines = hd.run(variant, ["readjplace"] + files)
    assert len(lines) == len(docs)
    return lines, files


def parse_read_line(line):
    toks = line.split(" ")
    assert toks[0] == "ok", line
    out = []
    for t in toks[2:]:
        parts = t.split(",")
        out.append((hd.unhex(parts[0]), [(int(e), float.fromhex(d), float.fromhex(q)) for e, d, q in (x.split(":") for x in parts[1:])]))
    assert int(toks[1]) == len(out)
    return out


VALID = ('{"tree": "(a,b,c);", "placements": [{"p": [[3, -10.5, 0.7, 0.25, 0.125], [0, -11.5, 0.3, 0.5, 1e-3]], "n": ["q1"]},\n'
         ' {"p": [[4294967295, -1, 1, 0, 2.5E+1]], "n": ["q2"]}], "metadata": {"invocation": "x", "deep": [[1, true, false, null]]},\n'
         ' "version": 3, "fields": ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "pendant_length"]}\n')


@pytest.mark.parametrize("variant", VARIANTS)
def test_reader_valid_documents(variant, tmp_path):
    deep = lambda n: "[" * n + "]" * n
    docs = [
        VALID,
        # fields in another order, with extra fields before, between and behind
        '{"fields": ["x", "pendant_length", "y", "distal_length", "likelihood", "edge_num", "z"],'
        ' "placements": [{"n": ["r"], "p": [[null, 0.5, "s", 0.25, -3, 7, [1, 2]]]}]}',
        # nm with a multiplicity, and no placements at all
        '{"fields": ["edge_num", "distal_length", "pendant_length"], "placements": [{"nm": [["r", 2.5]], "p": [[1, 2, 3]]}, {"n": ["e"], "p": []}]}',
        # every escape; \u of 1, 2 and 3 UTF-8 bytes
        '{"fields": ["edge_num", "distal_length", "pendant_length"], "placements": [{"n": ["a\\"b\\\\c\\/d\\be\\ff\\ng\\rh\\ti\\u0041\\u00e9\\u20ac\\u007f\\u0080\\u07ff\\u0800\\uffff"], "p": []}]}',
        # 64 levels of nesting below the top-level object are read
        '{"x": ' + deep(64) + ', "fields": ["edge_num", "distal_length", "pendant_length"], "placements": []}',
    ]
    lines, _ = read_lines(variant, tmp_path, docs)
    assert parse_read_line(lines[0]) == [(b"q1", [(3, 0.25, 0.125), (0, 0.5, 1e-3)]), (b"q2", [(4294967295, 0.0, 25.0)])]
    assert parse_read_line(lines[1]) == [(b"r", [(7, 0.25, 0.5)])]
    assert parse_read_line(lines[2]) == [(b"r", [(1, 2.0, 3.0)]), (b"e", [])]
    name = json.loads(docs[3])["placements"][0]["n"][0]
    assert parse_read_line(lines[3]) == [(name.encode("utf-8"), [])] and len("Aé€".encode()) == 6
    assert parse_read_line(lines[4]) == []


def number_start(text, k):
    """start of the number token that ends at byte k of text[:k], or k"""
    s = k
    while s > 0 and text[s - 1] in "0123456789+-.eE":
        s -= 1
    return s


@pytest.mark.parametrize("variant", VARIANTS)
def test_reader_refuses_a_file_cut_at_each_of_its_first_200_bytes(variant, tmp_path):
    assert len(VALID) > 210 and all(ord(c) < 128 for c in VALID)
    lines, files = read_lines(variant, tmp_path, [VALID[:k] for k in range(200)])
    for k, (line, f) in enumerate(zip(lines, files)):
        m = re.match(r"throw: (.*): malformed JSON at byte (\d+): ", line)
        assert m and m.group(1) == str(f), (k, line)
        # the offset is the end of the file, or the start of the number the cut went through ("1e", "-", "2.")
        assert int(m.group(2)) in (k, number_start(VALID, k)), (k, line)
        with pytest.raises(json.JSONDecodeError):
            json.loads(VALID[:k])


@pytest.mark.parametrize("variant", VARIANTS)
def test_reader_refuses_malformed_documents_by_offset_or_row(variant, tmp_path):
    head = '{"fields": ["edge_num", "distal_length", "pendant_length"], "placements": ['
    row = lambda r: head + '{"n": ["q0"], "p": [[1, 2, 3]]}, {"n": ["q1"], "p": [[1, 2, 3], ' + r + ']}]}'
    deep = '{"x": ' + "[" * 65 + "]" * 65 + "}"
    short_u = head + '{"n": ["\\u12'
    cases = [
        (head + '{"n": ["q"], "p": [[--, 2, 3]]}]}', r"malformed JSON at byte %d: bad number '--'" % (len(head) + 20)),
        (deep, r"malformed JSON at byte %d: nested too deeply" % (len('{"x": ') + 64)),
        (short_u, r"malformed JSON at byte %d: short \\u escape" % (len(short_u) - 2)),   # where the four digits should begin
        (head + '{"n": ["\\u12g4"], "p": []}]}', r"malformed JSON at byte \d+: bad \\u escape"),
        (head + '{"n": ["\\q"], "p": []}]}', r"malformed JSON at byte \d+: unknown escape"),
        (row("[1, 2]"), r"placement object 1: row 1: does not have one value per field"),
        (row("[1, 2, 3, 4]"), r"placement object 1: row 1: does not have one value per field"),
        (row("[1.5, 2, 3]"), r"placement object 1: row 1: edge_num is not a non-negative integer"),
        (row("[-1, 2, 3]"), r"placement object 1: row 1: edge_num is not a non-negative integer"),
        (row("[1e999, 2, 3]"), r"placement object 1: row 1: edge_num is not a non-negative integer"),
        (row("[4294967296, 2, 3]"), r"placement object 1: row 1: edge_num is not a non-negative integer"),
        (row('[1, "2", 3]'), r"placement object 1: row 1: \"distal_length\" is not a number"),
        (head + '{"n": ["a"], "nm": [["a", 1]], "p": []}]}', r"placement object 0: needs exactly one of \"n\" and \"nm\""),
        (head + '{"p": []}]}', r"placement object 0: needs exactly one of \"n\" and \"nm\""),
        (head + '{"n": ["a"], "p": []}, {"n": ["a", "b"], "p": []}]}', r"placement object 1: must carry exactly one name \(2 given\)"),
        (head + '{"n": [], "p": []}]}', r"placement object 0: must carry exactly one name \(0 given\)"),
        ('{"fields": ["edge_num", "distal_length"], "placements": []}', r"required field \"pendant_length\" is missing"),
        # a field named twice took the last one silently: refused, with both positions
        ('{"fields": ["edge_num", "distal_length", "pendant_length", "edge_num"], "placements": []}',
         r"field \"edge_num\" is named twice in \"fields\" \(entries 0 and 3\)"),
        ('{"fields": ["distal_length", "edge_num", "distal_length", "pendant_length"], "placements": []}',
         r"field \"distal_length\" is named twice in \"fields\" \(entries 0 and 2\)"),
        ('{"fields": ["edge_num", "distal_length", "pendant_length", "pendant_length"], "placements": []}',
         r"field \"pendant_length\" is named twice in \"fields\" \(entries 2 and 3\)"),
        (VALID + "x", r"malformed JSON at byte %d: text after the end of the document" % len(VALID)),
        ("", r"malformed JSON at byte 0: unexpected end of file"),
    ]
    lines, files = read_lines(variant, tmp_path, [d for d, _ in cases])
    for (doc, want), line, f in zip(cases, lines, files):
        assert line.startswith("throw: " + str(f) + ": ") and re.search(want, line), (doc[-60:], want, line)
    assert hd.run(variant, ["readjplace", tmp_path / "absent.jplace"])[0].startswith("throw: ")


# ---------------------------------------------------------------------------------------------------------------------
# trees
# ---------------------------------------------------------------------------------------------------------------------
LABELS = ["a", "b", "c", "d"]
SEQS = ["ACGTACGTAAGT", "ACGTTCGTACGA", "CCGTACTTACGT", "ACGAACGTACTT"]
SUBST = [1.0, 2.5, 0.5, 1.5, 3.0, 1.0]
FREQS = [0.3, 0.2, 0.2, 0.3]
MODEL = "GTR{1.0/2.5/0.5/1.5/3.0/1.0}+FU{0.3/0.2/0.2/0.3}"
T_VALID = "((a:0.1,b:0.2):0.05,c:0.3,d:0.4);"
DEF = "0.105360515657826"   # -ln 0.9, the default branch length (src/util/constants.hpp:12)


@pytest.fixture(scope="module")
def tree_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("trees")
    fa = d / "ref.fasta"
    fa.write_text("".join(">%s\n%s\n" % (l, s) for l, s in zip(LABELS, SEQS)))
    return d, fa


def oracle_lnl(newick, labels=LABELS, seqs=SEQS):
    from oracle_lib import Oracle
    o = Oracle(newick, labels, seqs, 4, SUBST, FREQS, [1.0])
    return o.tree_lnl(0), o.numbered_newick(6)


def run_trees(variant, tree_files, newicks, lnl=True, fasta=None, timeout=hd.RUN_TIMEOUT):
    d, fa = tree_files
    files = []
    for i, n in enumerate(newicks):
        f = d / ("t%s_%d.nwk" % (variant, i))
        f.write_text(n)
        files.append(f)
    lines = hd.run(variant, ["tree", fasta or fa, MODEL, "1" if lnl else "0"] + files, timeout=timeout)
    assert len(lines) == len(newicks)
    return lines


@pytest.mark.parametrize("variant", VARIANTS)
def test_trees_that_stay_valid(variant, tree_files):
    """a valid tree, the same without ';', the rooted form, a tree without lengths: branch count, the likelihood of the
    oracle (printed with six decimals: half a unit of the sixth, plus the oracle's own 1e-9) and its numbered newick"""
    rooted = "((a:0.1,b:0.2):0.02,(c:0.3,d:0.4):0.03);"
    nolen = "((a,b),c,d);"
    spaced = " ( ( a : 0.1 , b : 0.2 ) : 0.05 ,\n c : 0.3 , d : 0.4 ) ;\n"
    inner = "((a:0.1,b:0.2)ab:0.05,c:0.3,d:0.4)root;"
    lines = run_trees(variant, tree_files, [T_VALID, T_VALID[:-1], rooted, nolen, spaced, inner])
    want = [oracle_lnl(T_VALID), oracle_lnl(T_VALID), oracle_lnl("((a:0.1,b:0.2):0.05,c:0.3,d:0.4);"),
            oracle_lnl("((a:%s,b:%s):%s,c:%s,d:%s);" % ((DEF,) * 5)), oracle_lnl(T_VALID), oracle_lnl(inner)]
    for i, (line, (lnl, numbered)) in enumerate(zip(lines, want)):
        m = re.match(r"ok B=5 rooted=([01]) lnl=(-?[0-9.]+) (.*)$", line)
        assert m, line
        assert int(m.group(1)) == (1 if i == 2 else 0)
        assert abs(float(m.group(2)) - lnl) <= 5e-7 + 1e-9, (i, line, lnl)
        if i != 2:   # the rooted tree keeps its own edge numbering (checked against the reference's literals elsewhere)
            if i == 5:   # inner labels are printed back
                numbered = numbered.replace("):0.05", ")ab:0.05").replace(");", ")root;")
            assert m.group(3) == numbered, (i, line, numbered)
    assert "0.105361" in lines[3]
    assert lines[0] == lines[1] == lines[4]


@pytest.mark.parametrize("variant", VARIANTS)
def test_trees_that_are_refused(variant, tree_files):
    cases = [
        ("((a:0.1,b:0.2):0.05,c:0.3,d:0.4", r"expected ',' or '\)'"),            # cut before the last ')'
        ("((a:0.1,b:0.2):0.05,c:0.3,", r"empty tip label"),                        # cut before the last tip
        ("((a:0.1,b:0.2):0.05,c:0.3", r"expected ',' or '\)'"),
        ("(a:0.1,b:0.2,c:0.3,d:0.4);", r"multifurcations \(polytomies\)"),         # 4-way polytomy at the top
        ("((a:0.1,b:0.2,c:0.3):0.1,d:0.4,a:0.1);", r"multifurcations \(polytomies\)"),   # and inside
        ("((a:0.1):0.05,c:0.3,d:0.4);", r"unary node"),
        ("((a:0.1,e:0.2):0.05,c:0.3,d:0.4);", r"failed to find e$"),               # a tip that is no alignment row
        ("((a:0.1,a:0.2):0.05,c:0.3,d:0.4);", r"tip label 'a' appears more than once"),
        ("(a:0.1,c:0.3,d:0.4);", r"reference MSA sequence 'b' \(row 1\) is not a tip of the tree"),
        ("((a:1e400,b:0.2):0.05,c:0.3,d:0.4);", r"branch length '1e400' of 'a' is not a finite non-negative number"),
        ("((a:0.1,b:-0.2):0.05,c:0.3,d:0.4);", r"branch length '-0.2' of 'b' is not a finite non-negative number"),
        ("((a:0.1,b:0.2):nan,c:0.3,d:0.4);", r"branch length 'nan' is not a finite non-negative number"),
        ("((a:0.1,b:0.2):0.05,c:inf,d:0.4);", r"branch length 'inf' of 'c' is not a finite non-negative number"),
        ("", r"expected '\('"),
        ("((((((((((", r"empty tip label"),
        ("(('a':0.1,b:0.2):0.05,c:0.3,d:0.4);", r"quoted labels are not supported \(quote at byte 2\)"),
        ("((a:0.1,b:0.2):0.05,c[comment]:0.3,d:0.4);", r"bracket comments are not supported \('\[' at byte 21\)"),
        ("((a:0.1,b:0.2):0.05,\"c\":0.3,d:0.4);", r"quoted labels are not supported"),
        ("(a:0.1,b:0.2);", r"Number of tip nodes too small"),
        ("((a:0.1,b:0.2):0.05,(c:0.3,d", r"expected '\)'"),                       # a nesting that ends in mid-label
    ]
    lines = run_trees(variant, tree_files, [n for n, _ in cases])
    for (newick, want), line in zip(cases, lines):
        assert line.startswith("throw: ") and re.search(want, line), (newick, want, line)


@pytest.mark.parametrize("variant", VARIANTS)
def test_tree_ladder_of_65536_levels_and_a_nesting_cut_in_mid_label(variant, tree_files):
    """a caterpillar of 65 538 tips (65 536 nested '(') parses without recursion: 2n - 3 branches, and its numbered
    newick is never printed here.  The same nesting cut in the first label is refused, not a stack overflow."""
    d, _ = tree_files
    n = 65538
    fa = d / "ladder.fasta"
    if not fa.exists():
        fa.write_text("".join(">t%d\nAC%sT\n" % (i, "ACGT"[i % 4]) for i in range(n)))
    # top level: (<subtree>, t_{n-2}, t_{n-1})
    ladder = "(" * (n - 2) + "t0:0.1,t1:0.1)" + "".join(":0.01,t%d:0.1)" % i for i in range(2, n - 2)) + ":0.01,t%d:0.1,t%d:0.1);" % (n - 2, n - 1)
    assert ladder.count("(") == ladder.count(")") == n - 2
    cut = "(" * 65536 + "t0"
    lines = run_trees(variant, (d, fa), [ladder, cut], lnl=False, fasta=fa)
    assert lines[0] == "ok B=%d rooted=0 lnl=-" % (2 * n - 3), lines[0][:200]
    assert lines[1].startswith("throw: ") and "unary node or is malformed" in lines[1]


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
def max_cats():
    hdr = open(os.path.join(hd.ROOT, "include", "epa_dev.h")).read()
    return int(re.search(r"#define EPA_MAX_CATS (\d+)", hdr).group(1))


@pytest.mark.parametrize("variant", VARIANTS)
def test_model_descriptors_refused_with_the_parameter_named(variant):
    n = max_cats()
    assert n >= 4
    cases = [
        ("GTR+G4{-1}", r"\+G alpha must be a finite positive number \('-1' given\)"),   # looped for ever
        ("GTR+G4{0}", r"\+G alpha must be a finite positive number"),
        ("GTR+G4{-0.0}", r"\+G alpha must be a finite positive number"),
        ("GTR+G4{nan}", r"\+G alpha must be a finite positive number"),
        ("GTR+G4{inf}", r"\+G alpha must be a finite positive number"),
        ("GTR+G4{1e999}", r"\+G alpha"),
        ("GTR+G4a{-2}", r"\+G alpha must be a finite positive number"),
        ("GTR+G4{abc}", r"\+G alpha: 'abc' is not a number"),
        ("GTR+G4{}", r"\+G alpha: '' is not a number"),
        ("GTR+G0", r"\+G0: the number of rate categories must be 1 \.\. %d" % n),
        ("LG+G99999", r"\+G99999: the number of rate categories must be 1 \.\. %d" % n),
        ("LG+G%d" % (n + 1), r"\+G%d: the number of rate categories must be 1 \.\. %d" % (n + 1, n)),
        ("GTR+G99999999999999999999", r"the number of rate categories must be 1 \.\. %d" % n),
        ("GTR+R0{1}", r"\+R0: the number of rate categories must be 1 \.\. %d" % n),
        ("GTR+R%d{1}" % (n + 1), r"the number of rate categories must be 1 \.\. %d" % n),
        ("GTR{1/2/3}", r"Invalid number of substitution rates specified: 3 \(expected: 6\)"),
        ("GTR{1/2/3/4/5/6/7}", r"Invalid number of substitution rates specified: 7 \(expected: 6\)"),
        ("HKY{1/2/3}", r"Invalid number of substitution rates specified: 3 \(expected: 2\)"),
        ("PROTGTR{1/2}", r"Invalid number of substitution rates specified: 2 \(expected: 190\)"),
        ("GTR{1/x/3/4/5/6}", r"substitution rates: 'x' is not a number"),
        ("GTR+FU{0.25/0.25/0.5}", r"Invalid number of user frequencies specified: 3"),
        ("LG+FU{0.5/0.5}", r"Invalid number of user frequencies specified: 2"),
        ("GTR+FU{0.25/0.25/0.25/0.25/0.1}", r"Invalid number of user frequencies specified: 5"),
        ("GTR+R3{1/2}", r"Invalid number of free rates specified: 2 \(expected: 3\)"),
        ("GTR+R2{1/2}{0.5}", r"Invalid number of rate weights specified: 1 \(expected: 2\)"),
        ("GTR+I{1}", r"\+I p-inv must be in \[0, 1\) \('1' given\)"),
        ("GTR+I{-0.1}", r"\+I p-inv must be in \[0, 1\)"),
        ("GTR+IU{1.5}", r"\+IU p-inv must be in \[0, 1\)"),
        ("GTR+I{nan}", r"\+I p-inv must be in \[0, 1\)"),
        ("GTR+I", r"\+I needs an explicit value"),
        ("FOO+G4", r"Invalid model name: FOO"),
        ("GTRR", r"Invalid model name: GTRR"),
        ("", r"Invalid model name: the descriptor is empty"),
        ("+G4", r"Invalid model name: the descriptor is empty or begins with an option"),
        ("GTR{1/2/3/4/5/6", r"unbalanced '\{' in '\{1/2/3/4/5/6'"),
        ("GTR+G4{0.5", r"unbalanced '\{' in '\{0.5'"),
        ("GTR+FU{0.25/0.25", r"unbalanced '\{'"),
        ("GTR+X", r"option \+X is not supported"),
        ("GTR+G4+R2{1/2}", r"\+G and \+R are mutually exclusive"),
        ("GTR G4", r"Invalid model name: GTR G4"),
    ]
    lines = hd.run(variant, ["model"] + [c for c, _ in cases])   # hd.RUN_TIMEOUT: a hang fails the test
    assert len(lines) == len(cases)
    for (desc, want), line in zip(cases, lines):
        assert line.startswith("throw: ") and re.search(want, line), (desc, want, line)


def gamma_mean_rates(alpha, k):
    """category means of the discrete Gamma (Yang 1994) from the oracle's own routine"""
    from oracle_lib import gamma_rates
    return list(gamma_rates(alpha, k))


@pytest.mark.parametrize("variant", VARIANTS)
def test_model_descriptors_that_stay_valid(variant):
    n = max_cats()
    descs = ["GTR+G4{0.5}", "GTR+G1{2}", "GTR+G%d{0.3}" % n, "LG+G4{1.25}", "GTR+G{0.02}", "GTR+G4{100}", "JC", "HKY{1/4}+FU{0.1/0.2/0.3/0.4}+I{0.25}",
             "GTR+R2{1/3}{0.25/0.75}", "DNA", "GTR+I{0}"]
    lines = hd.run(variant, ["model"] + descs)
    got = {}
    for d, line in zip(descs, lines):
        m = re.match(r"ok cats=(\d+) states=(\d+) pinv=(\S+) rates=(\S+) (.*)$", line)
        assert m, (d, line)
        got[d] = (int(m.group(1)), int(m.group(2)), float.fromhex(m.group(3)), [float.fromhex(x) for x in m.group(4).split("/")], m.group(5))
    for d, alpha, k in (("GTR+G4{0.5}", 0.5, 4), ("GTR+G1{2}", 2.0, 1), ("GTR+G%d{0.3}" % n, 0.3, n), ("LG+G4{1.25}", 1.25, 4),
                        ("GTR+G{0.02}", 0.02, 4), ("GTR+G4{100}", 100.0, 4), ("DNA", 1.0, 4)):
        cats, states, _, rates, text = got[d]
        assert cats == k and states == (20 if d.startswith("LG") else 4)
        want = gamma_mean_rates(alpha, k)
        # mean 1 by construction; each category mean within the oracle's own quadrature error
        assert abs(sum(rates) / k - 1.0) < 1e-12
        assert all(abs(a - b) <= 1e-6 * max(b, 1e-3) for a, b in zip(rates, want)), (d, rates, want)
        if k > 1:
            assert ("+G%d{%.6f}" % (k, alpha)) in text
    assert got["JC"][0] == 1 and got["JC"][3] == [1.0]
    assert got["HKY{1/4}+FU{0.1/0.2/0.3/0.4}+I{0.25}"][2] == 0.25
    assert got["GTR+R2{1/3}{0.25/0.75}"][3] == [1.0 / 2.5, 3.0 / 2.5]
    assert got["GTR+I{0}"][2] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# FASTA, views, bfast
# ---------------------------------------------------------------------------------------------------------------------
WS = b" \t\n\v\f\r"


def plain_fasta(data):
    """records = '>' at the start of a line; header without trailing blanks / CR; sequence upper-cased, white space out"""
    recs, cur = [], None
    for line in data.split(b"\n"):
        if line.startswith(b">"):
            cur = [line[1:].rstrip(b"\r \t"), b""]
            recs.append(cur)
        elif cur is not None:
            cur[1] += bytes(c for c in line if c not in WS).upper()
    return [(h, s) for h, s in recs]


def parse_msa_line(line):
    toks = line.split(" ")
    assert toks[0] == "ok", line
    recs = [tuple(hd.unhex(x) for x in t.split(":")) for t in toks[2:2 + int(toks[1])]]
    return recs, toks[2 + int(toks[1]):]


FASTA_CASES = {
    "text before the first record": b"junk line\n\nmore > junk\n>a\nACGT\n>b\nGGTT\n",
    "records with empty sequences": b">a\n>b\nAC\n>c\n\n>d\n",
    "last record without a newline": b">a\nAC\n>b\nGT",
    "last record is a bare header": b">a\nAC\n>b",
    "CRLF line ends": b">a desc\r\nAC\r\nGT\r\n>b\r\nAA\r\n",
    "tabs and spaces inside a row": b">a \t\nAC GT\tAA \n  cc\n>b\n\tGG\n",
    "lower case and a '>' inside a line": b">a\nac>gt\n>b\nnn--\n",
    "empty file": b"",
    "no record at all": b"just text\n",
}


@pytest.mark.parametrize("variant", VARIANTS)
def test_fasta_reader_against_a_plain_parser(variant, tmp_path):
    names = list(FASTA_CASES)
    files = []
    for i, n in enumerate(names):
        f = tmp_path / ("f%d.fasta" % i)
        f.write_bytes(FASTA_CASES[n])   # real \r bytes
        files.append(f)
    for chunk in (1, 2, 1000):
        lines = hd.run(variant, ["fasta", chunk] + files)
        for n, line in zip(names, lines):
            assert parse_msa_line(line)[0] == plain_fasta(FASTA_CASES[n]), (n, chunk, line)
    assert hd.run(variant, ["fasta", 5, tmp_path / "absent.fasta"])[0].startswith("throw: file_check failed")


@pytest.mark.parametrize("variant", VARIANTS)
def test_read_next_views_hands_doubtful_chunks_to_the_parser(variant, tmp_path):
    """read_next_views takes record starts from a predicted stride.  (1) regular one-line records come as views.  (2) a
    short record plus the next record's header inside exactly `sites` bytes came out as ONE merged row, later refused as
    'char is invalid!' under the wrong name: it must come out of read_next as the records a plain parser sees, the
    short one on its own, which encode_chunk then refuses with the reference's 'Query sequence length not same as
    reference alignment!'.  (3) records that stop matching the stride half way."""
    sites = 12
    regular = b"".join(b">r%d\n%s\n" % (i, (b"ACGT" * 3)) for i in range(7))
    merged = (b">r0\nACGTACGTACGT\n>r1\nAAAACCCCGGGG\n" + b">r2\nACGT\n>r3\nACG\n" + b">r4\nTTTTACGTACGT\n>r5\nACGTACGTAAAA\n")
    assert len(b"ACGT\n>r3\nACG") == sites
    half = (b"".join(b">s%d\n%s\n" % (i, (b"ACGT" * 3)) for i in range(4)) + b"".join(b">s%d\nACGTAC\nGTACGT\n" % i for i in range(4, 8)))
    crlf = b"".join(b">c%d\r\n%s\r\n" % (i, (b"acgt" * 3)) for i in range(3))
    blobs = [regular, merged, half, crlf]
    files = []
    for i, b in enumerate(blobs):
        f = tmp_path / ("v%d.fasta" % i)
        f.write_bytes(b)
        files.append(f)
    for chunk in (100, 3, 2, 1):
        lines = hd.run(variant, ["views", sites, chunk] + files)
        for i, (blob, line) in enumerate(zip(blobs, lines)):
            recs, tail = parse_msa_line(line)
            assert recs == plain_fasta(blob), (i, chunk, line)
            counts = dict(t.split("=") for t in tail)
            if i in (0, 3):
                assert int(counts["views"]) > 0 and int(counts["read"]) == 0, (i, chunk, line)
    recs = plain_fasta(merged)
    assert [len(s) for _, s in recs] == [12, 12, 4, 3, 12, 12]


def bfast_bytes(records, mask=None, offsets=None, n=None):
    """the format read by Fasta_Stream::open_bfast: magic, count, [mask], (id, offset) table, records"""
    nt = "-TGKCYSBAWRDMHVN"
    body, offs = b"", []
    table_at = 7 + 8 + (8 + len(mask) if mask is not None else 0)
    data_at = table_at + 16 * len(records)
    for h, s in records:
        offs.append(data_at + len(body))
        codes = [nt.index(c) for c in s] + [0]
        body += struct.pack("<Q", len(h)) + h.encode() + struct.pack("<Q", len(s))
        body += bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(s), 2))
    offs = offsets(offs) if offsets else offs
    out = b"BFAST\0\0" + struct.pack("<Q", len(records) if n is None else n)
    if mask is not None:
        out += struct.pack("<Q", len(mask)) + mask.encode()
    for i, o in enumerate(offs):
        out += struct.pack("<QQ", i, o)
    return out + body, table_at, data_at


BF_RECORDS = [("q0", "ACGT-N"), ("q1 desc", "--GTAC"), ("q2", "NNNNNN"), ("q3", "TTTTTA")]
BF_GAPS = BF_RECORDS[:2] + [("q2", "------")] + BF_RECORDS[3:]


@pytest.mark.parametrize("variant", VARIANTS)
def test_bfast_reader_valid_cut_and_out_of_range(variant, tmp_path):
    want = [(h.encode(), s.encode()) for h, s in BF_RECORDS]
    files, expect = [], []

    def add(name, blob, check):
        f = tmp_path / (name + ".bfast")
        f.write_bytes(blob)
        files.append(f)
        expect.append((name, check))
    for mask in (None, "000000"):
        tag = "m" if mask else "p"
        blob, table_at, data_at = bfast_bytes(BF_RECORDS, mask)
        add("valid_" + tag, blob, want)
        # cut at every 8-byte boundary of the header and the offset table (the magic is 7 bytes long)
        for cut in range(7, data_at + 1, 8):
            add("cut_%s_%d" % (tag, cut), blob[:cut], r"bfast|Binary_Fasta")
        add("cut_last_record_" + tag, blob[:-2], r"bfast: truncated sequence \(record 3 at offset %d\)" % (len(blob) - 21))
        # an offset beyond the file: the second record's
        far, _, _ = bfast_bytes(BF_RECORDS, mask, offsets=lambda o: [o[0], len(blob) + 100] + o[2:])
        add("far_" + tag, far, r"bfast: bad sequence offset \(record 1 at offset %d\)" % (len(blob) + 100))
        near, _, _ = bfast_bytes(BF_RECORDS, mask, offsets=lambda o: o[:3] + [len(blob) - 8])
        add("near_" + tag, near, r"bfast: .* \(record 3 at offset %d\)" % (len(blob) - 8))
    # a count no file of this size can hold, a header length and a site count beyond the file
    blob, table_at, data_at = bfast_bytes(BF_RECORDS)
    add("count", blob[:7] + struct.pack("<Q", 1 << 40) + blob[15:], r"bfast: the header announces %d sequences" % (1 << 40))
    add("hlen", blob[:data_at] + struct.pack("<Q", 1 << 50) + blob[data_at + 8:], r"bfast: truncated header \(record 0 at offset %d\)" % data_at)
    add("sites", blob[:data_at + 10] + struct.pack("<Q", 1 << 50) + blob[data_at + 18:], r"bfast: truncated sequence \(record 0 at offset %d\)" % data_at)
    for chunk in (1, 3, 100):
        lines = hd.run(variant, ["fasta", chunk] + files)
        for (name, check), line in zip(expect, lines):
            if isinstance(check, list):
                assert parse_msa_line(line)[0] == check, (name, line)
            else:
                assert line.startswith("throw: ") and re.search(check, line), (name, check, line)


@pytest.mark.parametrize("variant", VARIANTS)
def test_bfast_wire_rows_valid_cut_and_out_of_range(variant, tmp_path):
    """read_next_wire reads the mapped file directly: the same malformed files, every offset and length held against the
    mapping's size before it is followed"""
    nt = "-TGKCYSBAWRDMHVN"
    blob, table_at, data_at = bfast_bytes(BF_RECORDS)
    far, _, _ = bfast_bytes(BF_RECORDS, offsets=lambda o: [o[0], len(blob) + 100] + o[2:])
    edge, _, _ = bfast_bytes(BF_RECORDS, offsets=lambda o: o[:3] + [len(blob) - 8])
    hlen = blob[:data_at] + struct.pack("<Q", 1 << 50) + blob[data_at + 8:]
    width = blob[:data_at + 10] + struct.pack("<Q", 1 << 50) + blob[data_at + 18:]
    blobs = [blob, far, edge, hlen, width, blob[:-2]]
    files = []
    for i, b in enumerate(blobs):
        f = tmp_path / ("w%d.bfast" % i)
        f.write_bytes(b)
        files.append(f)
    for chunk in (1, 100):
        lines = hd.run(variant, ["wire", 6, chunk, 0] + files)
        toks = lines[0].split(" ")
        assert toks[:3] == ["ok", "4", "bfast"]
        for (h, s), t in zip(BF_RECORDS, toks[3:]):
            hh, b, span, codes = t.split(":")
            assert hd.unhex(hh) == h.encode() and (int(b), int(span)) == (0, 6)
            assert "".join(nt[x >> 4] + nt[x & 15] for x in hd.unhex(codes)) == s
        assert re.match(r"throw: bfast: truncated sequence \(record 1 at offset %d\)" % (len(blob) + 100), lines[1]), lines[1]
        assert re.match(r"throw: bfast: truncated sequence \(record 3 at offset %d\)" % (len(blob) - 8), lines[2]), lines[2]
        assert re.match(r"throw: bfast: truncated sequence \(record 0 at offset %d\)" % data_at, lines[3]), lines[3]
        assert lines[4] == "throw: Query sequence length not same as reference alignment!", lines[4]
        assert re.match(r"throw: bfast: truncated sequence \(record 3 ", lines[5]), lines[5]
    # premasking: the window of every record, an all-gap record refused by name
    (tmp_path / "gaps.bfast").write_bytes(bfast_bytes(BF_GAPS)[0])
    lines = hd.run(variant, ["wire", 6, 100, 1, tmp_path / "gaps.bfast"])
    assert lines[0] == "throw: Sequence with header 'q2' does not appear to have any non-gap sites!", lines[0]
    two, _, _ = bfast_bytes(BF_RECORDS[:2])
    (tmp_path / "two.bfast").write_bytes(two)
    toks = hd.run(variant, ["wire", 6, 100, 1, tmp_path / "two.bfast"])[0].split(" ")
    assert [t.split(":")[1:3] for t in toks[3:]] == [["0", "6"], ["2", "4"]]


# ---------------------------------------------------------------------------------------------------------------------
# FASTQ
# ---------------------------------------------------------------------------------------------------------------------
def fq(*recs):
    return b"".join(b"@%s\n%s\n+\n%s\n" % r for r in recs)


@pytest.mark.parametrize("variant", VARIANTS)
def test_fastq_reader_valid_and_malformed(variant, tmp_path):
    good = [(b"r1", b"AC-gt", b"II!~#"), (b"r2 x", b"--NTN", b"!!5I~")]
    valid = fq(*good)
    cases = [
        ("valid", valid, good),
        ("crlf", valid.replace(b"\n", b"\r\n"), good),
        ("no last newline", valid[:-1], good),
        ("blank lines between records", valid.replace(b"\n@r2", b"\n\n\n@r2"), good),
        ("empty file", b"", []),
        ("quality shorter", fq(good[0], (b"r2", b"ACGTA", b"IIII")), r"FASTQ record 2 \('r2'\): the read has 5 columns, its quality line 4 "),
        ("quality longer", fq((b"r1", b"ACGTA", b"IIIIII")), r"FASTQ record 1 \('r1'\): the read has 5 columns, its quality line 6 "),
        ("quality below '!'", fq(good[0], (b"r2", b"ACGTA", b"II\x1fII")), r"FASTQ record 2 \('r2'\): a quality character lies outside"),
        ("quality above '~'", fq((b"r1", b"ACGTA", b"II\x7fII")), r"FASTQ record 1 \('r1'\): a quality character lies outside"),
        ("quality byte 0xff", fq((b"r1", b"ACGTA", b"II\xffII")), r"FASTQ record 1 \('r1'\): a quality character lies outside"),
        ("missing +", valid + b"@r3\nACGTA\nIIIII\n@r4\n", r"FASTQ record 3 \('r3'\): the third line does not begin with '\+'"),
        ("no @", valid + b"r3\nACGTA\n+\nIIIII\n", r"FASTQ record 3: the header line does not begin with '@'"),
        ("cut in line 1", valid + b"@r", r"FASTQ record 3 \('r'\): the record is incomplete"),
        ("cut in line 2", valid + b"@r3\nAC", r"FASTQ record 3 \('r3'\): the record is incomplete"),
        ("cut in line 3", valid + b"@r3\nACGTA\n+", r"FASTQ record 3 \('r3'\): the record is incomplete"),
        ("cut after line 3", valid + b"@r3\nACGTA\n+\n", r"FASTQ record 3 \('r3'\): the record is incomplete"),
        ("cut in line 4", valid + b"@r3\nACGTA\n+\nIII", r"FASTQ record 3 \('r3'\): the read has 5 columns, its quality line 3 "),
    ]
    files = []
    for i, (_, blob, _) in enumerate(cases):
        f = tmp_path / ("q%d.fastq" % i)
        f.write_bytes(blob)
        files.append(f)
    for chunk in (1, 100):
        lines = hd.run(variant, ["fastq", chunk] + files)
        for (name, blob, want), line, f in zip(cases, lines, files):
            if isinstance(want, list):
                toks = line.split(" ")
                assert toks[0] == "ok" and int(toks[1]) == len(want), (name, line)
                assert toks[2] == "fastq=%d" % (1 if blob else 0)
                recs = [tuple(hd.unhex(x) for x in t.split(":")) for t in toks[3:3 + len(want)]]
                assert recs == [(h, s.upper(), q) for h, s, q in want], (name, line)
                if want:   # fastq_msa_info: columns that are a gap character in every read
                    assert toks[-2:] == ["sites=5", "mask=00100"], (name, line)
            else:
                assert line.startswith("throw: " + str(f) + ": ") and re.search(want, line), (name, want, line)
