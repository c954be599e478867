"""A function with external linkage that is not a kernel is declared in exactly one header, and the unit that defines it includes
that header; no .hip / .cpp file declares a function of another unit ("where a unit's interface is declared").

Two halves over the files named in SRCS of owshen_amd/csrc/Makefile plus verify_only.cpp:
  (a) the compiler: a host-only -Wmissing-prototypes pass names only kernels (k_*).  A definition that no header declares -- or
      whose header copy has drifted into a second overload -- is named.  Before the headers existed the pass named 82 functions
      that are not kernels, in 15 files.
  (b) the text: no source file holds a column-0, non-static function declaration.  The pattern below, applied to the sources as they
      were before the headers existed, found exactly the 75 hand-copied prototypes: capi.hip 41, groth16.hip 11, msm.hip 10,
      multi.hip 9, keygen.hip 3, verify_only.cpp 1 (and not the `static` forward declaration of prove_finish in groth16.hip).  Now: 0.
The link half of the rule is -Wl,-z,defs on the three link lines of the Makefile: a prototype that nobody defines fails the build."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "owshen_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# return type and qualifiers (no parenthesis, no '=', not `static`), a name, a parameter list that may span lines and may hold one
# level of parentheses, then `;` -- a definition has `{` there and a call does not start at column 0 with a type in front of it
DECL = re.compile(r"^(?!static\b|typedef\b|using\b|return\b)[A-Za-z_][^;{}()=#]*?[\s*&](\w+)\s*\((?:[^;{}()]|\([^;{}()]*\))*\)\s*;", re.M)


def _sources():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.+)$", mk, flags=re.M).group(1).split()
    assert len(srcs) >= 19 and "capi.hip" in srcs, srcs
    return srcs + ["verify_only.cpp"]


def _without_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def declarations(text):
    """(line, name) of every column-0, non-static function declaration in a source text"""
    text = _without_comments(text)
    return [(text.count("\n", 0, m.start()) + 1, m.group(1)) for m in DECL.finditer(text)]


def test_the_pattern_sees_a_prototype_and_only_a_prototype():
    text = """\
namespace og {
int pk_load(og_ctx*, const uint8_t*, size_t, og_pk**);   // 2
int assemble_g1(og_ctx*, const uint8_t*,
                uint8_t*, const uint8_t*);
int assemble_g2(og_ctx*, size_t, uint8_t*, bool wave_per_proof = false);
std::string get_error();
const char* name_of(uint32_t f);
void walk(void (*fn)(int), int n);
static int prove_finish(og_job* job, size_t* first_bad);
// int commented_out(int);
constexpr int N = pick(3);
int defined_here(int a) { return a; }
int defined_later(int a,
                  int b) {
  return helper(a, b);
}
using namespace og;
#define LAUNCH(k) run(k);
}
"""
    assert declarations(text) == [(2, "pk_load"), (3, "assemble_g1"), (5, "assemble_g2"), (6, "get_error"), (7, "name_of"), (8, "walk")]


def test_no_source_file_declares_a_function():
    found = {}
    for fn in _sources():
        hits = declarations(open(os.path.join(CSRC, fn)).read())
        if hits:
            found[fn] = hits
    assert not found, f"declare these in the header of the unit that defines them: {found}"


def _missing_prototypes(fn):
    p = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-fsyntax-only", "-Wmissing-prototypes", fn],
                       cwd=CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return fn, re.findall(r"warning: no previous prototype for function '([^']+)'", p.stderr)


def test_every_external_function_but_the_kernels_has_a_prototype_in_a_header():
    with ThreadPoolExecutor(max_workers=8) as pool:
        named = dict(pool.map(_missing_prototypes, _sources()))
    assert any(named.values()), "the pass named no kernel at all: is -Wmissing-prototypes still understood?"
    undeclared = {fn: [n for n in names if not n.startswith("k_")] for fn, names in named.items()}
    undeclared = {fn: names for fn, names in undeclared.items() if names}
    assert not undeclared, f"external functions without a prototype in a header (make them static, or declare them once): {undeclared}"
