"""csrc/internal.h is the one place where the library's translation units declare what they share (no GPU, no compiler:
a textual scan of the sources).

A hand-written prototype in a .hip file is checked against its definition only by the linker (a changed parameter list
shows up as an unresolved mangled name; a changed default argument or variable type not at all), so:
  1. every .hip of the Makefile's SRCS reaches internal.h (through common.h, the one way in);
  2. no .hip declares, at namespace scope, a function without a body that another .hip defines;
  3. no .hip holds an `extern` declaration other than `extern "C"` (dynamic `extern __shared__` arrays live inside
     kernels, not at namespace scope).
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monopsr_amd", "csrc")


def _srcs():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*\.hip.*)$", mk, re.M).group(1).split()
    assert len(srcs) >= 20 and all(s.endswith(".hip") for s in srcs), srcs
    return srcs


def _strip(text):
    """the source without comments, string / character literals and preprocessor lines"""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', lambda m: '"C"' if m.group(0) == '"C"' else '""', text)
    text = re.sub(r"'(?:\\.|[^'\\\n])'", "0", text)
    text = re.sub(r"(?m)^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text)
    return text


def _namespace_scope(text):
    """(declarations, definitions) at namespace scope of stripped source `text`: the text of every statement that
    ends in `;`, and the head (text in front of the body) of everything that has a body.  The braces of `namespace`
    and `extern "C"` blocks open no body."""
    decls, heads, stmt, depth, i = [], [], [], 0, 0
    while i < len(text):
        c = text[i]
        if c == "{":
            head = "".join(stmt).strip()
            if depth == 0 and re.match(r'^(?:inline\s+)?namespace\b[\w\s:]*$|^extern\s+"C"$', head):
                stmt = []
            else:
                if depth == 0:
                    heads.append(head)
                depth += 1
        elif c == "}":
            if depth > 0:
                depth -= 1
                if depth == 0:
                    # `= {...};` and `struct {...};` end in a semicolon that belongs to the same statement
                    j = i + 1
                    while j < len(text) and text[j].isspace():
                        j += 1
                    if j < len(text) and text[j] == ";":
                        i = j
                    stmt = []
        elif depth == 0:
            if c == ";":
                decls.append("".join(stmt).strip())
                stmt = []
            else:
                stmt.append(c)
        i += 1
    return decls, heads


def _function_name(head):
    """the name of the function that `head` declares, or None (variables, types, using-declarations, ...)"""
    head = re.sub(r"__attribute__\s*\(\((?:[^()]|\([^()]*\))*\)\)|__launch_bounds__\s*\([^()]*\)", " ", head)
    if re.match(r"^\s*(?:using|typedef|static_assert)\b", head) or "=" in head.split("(")[0]:
        return None
    if re.search(r"\b(?:struct|class|enum|union)\s+\w+\s*(?::[^()]*)?$", head):
        return None
    m = re.search(r"([A-Za-z_]\w*)\s*\(", head)
    return m.group(1) if m else None


def _scan():
    out = {}
    for src in _srcs():
        decls, heads = _namespace_scope(_strip(open(os.path.join(CSRC, src)).read()))
        out[src] = (decls, {n for n in map(_function_name, heads) if n})
    return out


def test_every_source_reaches_the_internal_header():
    common = open(os.path.join(CSRC, "common.h")).read()
    assert re.search(r'^#include "internal\.h"', common, re.M)
    assert os.path.exists(os.path.join(CSRC, "internal.h"))
    for src in _srcs():
        text = open(os.path.join(CSRC, src)).read()
        assert re.search(r'^#include "common\.h"', text, re.M), src
        assert not re.search(r'^#include "internal\.h"', text, re.M), "%s: internal.h comes through common.h" % src


def test_no_cross_file_prototype_in_a_source():
    scan = _scan()
    for src, (decls, _) in scan.items():
        elsewhere = set().union(*(names for other, (_, names) in scan.items() if other != src))
        for d in decls:
            name = _function_name(d) if d.endswith(")") else None
            assert name is None or name not in elsewhere, "%s re-declares %s: it belongs in internal.h" % (src, name)


def test_no_extern_declaration_in_a_source():
    for src, (decls, heads) in _scan().items():
        for d in list(decls) + list(heads):
            assert not re.match(r'^extern\b(?!\s*"C")', d), "%s: '%s' belongs in internal.h" % (src, d[:80])


def test_the_scan_sees_what_it_is_meant_to_see():
    decls, heads = _namespace_scope(_strip(
        'namespace a {\nint f(int x, const char *s = ")");  // g();\nextern int v;\nextern "C" int c(void) { return f(1); }\n'
        "static int t[2] = {1, 2};\n__global__ __launch_bounds__(256) void k(int n) { if (n) { h(); } }\n}\n"))
    assert [_function_name(d) for d in decls] == ["f", None] and decls[1] == "extern int v"
    assert sorted(filter(None, map(_function_name, heads))) == ["c", "k"]
