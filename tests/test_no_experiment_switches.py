"""The mapping library carries no experiment switches: what genefuserust_amd/csrc compiles does not depend on a -D, and
what gfmatch.hip reads from the environment is documented.  An experiment lives on a branch (NOTEBOOK.md, top).  Reads
files only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genefuserust_amd", "csrc")


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(files) >= 10 and os.path.join(CSRC, "gfmatch.hip") in files
    return files


def _logical_lines(text):
    """Source lines with backslash continuations joined and comments removed."""
    text = re.sub(r"/\*.*?\*/", " ", text.replace("\\\n", " "), flags=re.S)
    return [re.sub(r"//.*", "", l) for l in text.split("\n")]


def test_preprocessor_conditionals_test_compiler_macros_only():
    seen = 0
    for path in _sources():
        for n, line in enumerate(_logical_lines(open(path).read()), 1):
            m = re.match(r"\s*#\s*(ifdef|ifndef|if|elif)\b(.*)", line)
            if not m:
                continue
            seen += 1
            names = [x for x in re.findall(r"[A-Za-z_]\w*", m.group(2)) if x != "defined"]
            assert names, "%s:%d: a conditional on a constant: %s" % (os.path.basename(path), n, line.strip())
            for x in names:
                assert x.startswith("__"), "%s:%d: conditional on %s, which a -D could set: %s" % (
                    os.path.basename(path), n, x, line.strip())
    assert seen >= 3  # (__HIPCC__, __HIP_DEVICE_COMPILE__, __x86_64__: the scan does find conditionals)


def test_every_environment_variable_read_is_documented():
    # every file of csrc/ (the headers read nothing today), and secure_getenv and the like as well as getenv
    src = "\n".join("\n".join(_logical_lines(open(path).read())) for path in _sources())
    calls = re.findall(r"getenv\s*\(([^)]*)\)", src)
    assert len(calls) >= 8
    names = set()
    for arg in calls:
        m = re.fullmatch(r'\s*"(\w+)"\s*', arg)
        assert m, "getenv of something that is not a string literal: %r" % arg
        names.add(m.group(1))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 7. Environment"):]
    sec = sec[:sec.index("\n## ", 4)]
    documented = set(re.findall(r"^\|\s*`(\w+)`\s*\|", sec, flags=re.M))
    assert names <= documented, "read by csrc/ but not in INTEGRATION.md's environment table: %s" % sorted(names - documented)
