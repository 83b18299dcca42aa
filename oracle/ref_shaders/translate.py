"""Turns the reference's sampler-free GLSL include files into C++ that compiles against glsl_compat.h.

The translation is textual and small on purpose, so that what is compiled is still the reference's own text:
  - comments are dropped (nothing of them is needed, and `in` / `out` occur in them as words);
  - #extension and #include lines are dropped; the files are concatenated in dependency order instead;
  - `inout T x` and `out T x` become `T& x`, `in T x` becomes `T x`;
  - a literal with a decimal point or an exponent gets an `f`: in GLSL it is a float, in C++ it would be a double and
    would turn the arithmetic around it into double arithmetic;
  - the swizzles that occur (.xy .xz .rgb) become calls;
  - a vector constructor vec3(a, b, c) becomes vec3{a, b, c}: GLSL evaluates arguments left to right, C++ only promises that
    for a braced list, and vec3(randomFloat(s), randomFloat(s), randomFloat(s)) draws in that order;
  - pbr_lighting.glsl is cut before imageBasedLighting, which needs samplers.
The output goes to oracle/_ref/, which git ignores: neither the reference's text nor anything made from it is committed.
"""
import os
import re

FILES = ("random.glsl", "restir_sampling.glsl", "brdf.glsl", "pbr_lighting.glsl", "atmosphere.glsl")
CUT_BEFORE = {"pbr_lighting.glsl": "vec3 imageBasedLighting"}

_FLOAT = re.compile(r"(?<![\w.])(\d+\.\d*(?:[eE][+-]?\d+)?|\.\d+(?:[eE][+-]?\d+)?|\d+[eE][+-]?\d+)(?![\w.])")


def _brace_constructors(text):
    out, i = [], 0
    pat = re.compile(r"\b(u?vec[234])\(")
    while True:
        m = pat.search(text, i)
        if m is None:
            return "".join(out) + text[i:]
        depth, j = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        out.append(text[i:m.start()] + m.group(1) + "{" + _brace_constructors(text[m.end():j - 1]) + "}")
        i = j


def translate_text(name, text):
    cut = CUT_BEFORE.get(name)
    if cut is not None:
        at = text.index(cut)
        text = text[:at]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^[ \t]*#[ \t]*(extension|include)\b[^\n]*\n", "", text, flags=re.M)
    text = re.sub(r"\b(?:inout|out)\s+(\w+)\s+(\w+)", r"\1& \2", text)
    text = re.sub(r"\bin\s+(\w+)\s+(\w+)", r"\1 \2", text)
    text = _FLOAT.sub(r"\1f", text)
    text = re.sub(r"\.(xy|xz|rgb)\b", r".\1()", text)
    text = _brace_constructors(text)
    text = re.sub(r"\n\s*\n+", "\n", text)
    return text


def translate(include_dir):
    """-> the C++ text of the five files, each under a '// ---- name' line"""
    parts = ["// made by oracle/ref_shaders/translate.py from the reference's shaders/include; not to be committed\n"]
    for name in FILES:
        with open(os.path.join(include_dir, name)) as f:
            parts.append("// ---- %s\n%s\n" % (name, translate_text(name, f.read())))
        if name == "pbr_lighting.glsl":
            parts.append("#undef INFINITY\n")  # <cmath>'s, which atmosphere.glsl defines again (and never uses)
    return "".join(parts)
