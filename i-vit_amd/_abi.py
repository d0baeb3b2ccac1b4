"""include/ivit.h, include/ivit_eval.h, include/ivit_features.h, include/ivit_attnmap.h, include/ivit_classmap.h, include/ivit_hidden.h, include/ivit_search.h, include/ivit_modelfile.h, include/ivit_probe.h, include/ivit_views.h, include/ivit_cluster.h, include/ivit_range.h and include/ivit_jpeg.h, each parsed once: the only statement of the C-ABI that Python reads.  _lib.py binds libivit_hip.so from them,
tools/gen_twin_header.py prints the CPU twin's prototypes from it, the tests bind the twin and walk the entry points through it.
Standard library only, so a tool loads this file without the package (and without torch).

    ABI.functions   name -> Function(ret, params, text): ret and every parameter a Decl; text is the parameter list as written,
                    whitespace normalised (what the twin header prints)
    ABI.structs     name -> [Decl, ...] in declaration order
    ABI.handles     names of the opaque handles (typedef struct X *name;)
    ABI.constants   the enum's values and the integer #defines (IVIT_VERSION)
    EVAL_ABI        the same of include/ivit_eval.h, the second public header: ITS functions and constants (IVIT_EVAL_VERSION), with
                    the handles and structs of ivit.h, which it includes, known to it
    FEATURES_ABI    the same of include/ivit_features.h, the third public header (IVIT_FEATURES_VERSION and the two modes)
    ATTNMAP_ABI     the same of include/ivit_attnmap.h, the fourth (IVIT_ATTNMAP_VERSION and the two modes of the fp32 map)
    CLASSMAP_ABI    the same of include/ivit_classmap.h, the fifth (IVIT_CLASSMAP_VERSION and the two modes of the runner)
    HIDDEN_ABI      the same of include/ivit_hidden.h, the sixth (IVIT_HIDDEN_VERSION and the two layouts of the fp32 form)
    SEARCH_ABI      the same of include/ivit_search.h, the seventh (IVIT_SEARCH_VERSION)
    MODELFILE_ABI   the same of include/ivit_modelfile.h, the eighth (IVIT_MODELFILE_VERSION); it declares a handle (ivit_model) and a
                    struct (ivit_model_info) of its own, listed behind those of ivit.h
    PROBE_ABI       the same of include/ivit_probe.h, the ninth (IVIT_PROBE_VERSION)
    VIEWS_ABI       the same of include/ivit_views.h, the tenth (IVIT_VIEWS_VERSION); it declares a struct (ivit_view_desc) of its own,
                    listed behind those of ivit.h
    CLUSTER_ABI     the same of include/ivit_cluster.h, the eleventh (IVIT_CLUSTER_VERSION)
    RANGE_ABI       the same of include/ivit_range.h, the twelfth (IVIT_RANGE_VERSION)
    JPEG_ABI        the same of include/ivit_jpeg.h, the thirteenth (IVIT_JPEG_VERSION); it declares a struct (ivit_jpeg_desc) of its own
                    with fixed-size array members, listed behind those of ivit.h

A Decl is (name, base, ptr, array, type): base type name, pointer depth, array length or None, and the type as text.

The mapping to ctypes, one rule for parameters and fields alike:
  - int, the intN_t / uintN_t types, float, double and size_t map to their ctypes types; an array field to (that type) * length;
  - a struct by value maps to its generated Structure;
  - every pointer maps to c_void_p, and so does every array parameter and every opaque handle: a device address and a host address
    have the same C type, and c_void_p takes what callers pass (byref(...), ctypes arrays, pointer instances, ints, None);
  - `const char *` as a return type maps to c_char_p.

A declaration this parser does not understand — an unknown base type, a function pointer, a bit-field, a union, implicit enum values —
raises AbiError naming the declaration: it never guesses and never skips."""
import collections
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ivit.h")
EVAL_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_eval.h")
FEATURES_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_features.h")
ATTNMAP_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_attnmap.h")
CLASSMAP_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_classmap.h")
HIDDEN_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_hidden.h")
SEARCH_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_search.h")
MODELFILE_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_modelfile.h")
PROBE_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_probe.h")
VIEWS_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_views.h")
CLUSTER_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_cluster.h")
RANGE_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_range.h")
JPEG_HEADER = os.path.join(os.path.dirname(HEADER), "ivit_jpeg.h")

Decl = collections.namedtuple("Decl", "name base ptr array type")
Function = collections.namedtuple("Function", "ret params text")
Abi = collections.namedtuple("Abi", "functions structs handles constants")

SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           **{f"{u}int{n}_t": getattr(ctypes, f"c_{u}int{n}") for u in ("", "u") for n in (8, 16, 32, 64)}}
POINTER_ONLY = {"void", "char"}          # base types that exist behind a pointer only


class AbiError(ValueError):
    pass


def _declarators(text, abi, what):
    """`const T *a`, `T a, b`, `T a[4]` -> [Decl, ...]"""
    m = re.fullmatch(r"(const )?(\w+)\b ?(.*)", text)
    if not m:
        raise AbiError(f"include/ivit.h: cannot parse {what} `{text}`")
    const, base, rest = m.group(1) or "", m.group(2), m.group(3)
    if base not in SCALARS and base not in POINTER_ONLY and base not in abi.structs and base not in abi.handles:
        raise AbiError(f"include/ivit.h: unknown type `{base}` in {what} `{text}`")
    out = []
    for d in rest.split(","):
        m = re.fullmatch(r" ?((?:\* ?)*)(\w+) ?(?:\[ ?(\d+) ?\])?", d)
        if not m:                        # a function pointer, a bit-field, `* const`, a missing name
            raise AbiError(f"include/ivit.h: cannot parse {what} `{text}`")
        ptr, array = m.group(1).count("*"), int(m.group(3)) if m.group(3) else None
        if base in POINTER_ONLY and not ptr:
            raise AbiError(f"include/ivit.h: `{base}` by value in {what} `{text}`")
        out.append(Decl(m.group(2), base, ptr, array, const + base + (" " + "*" * ptr if ptr else "") + (f" [{array}]" if array else "")))
    return out


def _one(text, abi, what):
    ds = _declarators(text, abi, what)
    if len(ds) != 1:
        raise AbiError(f"include/ivit.h: cannot parse {what} `{text}`")
    return ds[0]


def _function(decl, abi):
    m = re.fullmatch(r"(.*?) ?(\w+) ?\((.*)\)", decl)
    if not m or "(" in m.group(3):
        raise AbiError(f"include/ivit.h: cannot parse declaration `{decl}`")
    ret = _one(m.group(1) + " " + m.group(2), abi, "prototype")
    if ret.array or ret.base in abi.structs or (ret.ptr and ret.type != "const char *"):
        raise AbiError(f"include/ivit.h: return type of `{decl}` is neither a scalar, a handle nor `const char *`")
    text = m.group(3).strip()
    params = [_one(p.strip(), abi, f"parameter of {ret.name}") for p in ([] if text == "void" else text.split(","))]
    return Function(ret, params, text)


def parse(text, base=None):
    """the declarations of a header in the dialect of include/ivit.h -> Abi.  `base`: the Abi of a header this one includes — its
    handles and structs are known types here (and listed in the result, so that ctype() maps them); functions and constants are
    this header's own"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    if "/*" in text:
        raise AbiError(f"include/ivit.h: unterminated comment `{text[text.index('/*'):][:80]}`")
    abi = Abi(collections.OrderedDict(), collections.OrderedDict(base.structs if base else ()), list(base.handles if base else ()),
              collections.OrderedDict())
    lines = []
    for line in text.split("\n"):
        if line.lstrip().startswith("#"):                    # preprocessor: an integer #define is a constant, a macro is refused
            m = re.fullmatch(r"\s*#\s*define\s+(\w+)\s*(.*?)\s*", line)
            if m and m.group(2):
                if not re.fullmatch(r"-?\d+", m.group(2)):
                    raise AbiError(f"include/ivit.h: cannot parse `{line.strip()}`")
                abi.constants[m.group(1)] = int(m.group(2))
        else:
            lines.append(line)
    text = " ".join("\n".join(lines).split())
    m = re.search(r'extern "C" \{', text)
    if m:                                                    # the guarded extern "C" block: its braces hold no declaration
        if not text.endswith("}"):
            raise AbiError('include/ivit.h: extern "C" { is not closed at the end of the header')
        text = text[:m.start()] + text[m.end():-1]
    decls, depth, start = [], 0, 0
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            decls.append(text[start:i].strip())
            start = i + 1
    if text[start:].strip():
        raise AbiError(f"include/ivit.h: unterminated declaration `{text[start:].strip()[:80]}`")
    for decl in decls:
        m = re.fullmatch(r"typedef struct \w+ ?\* ?(\w+)", decl)
        if m:
            abi.handles.append(m.group(1))
            continue
        m = re.fullmatch(r"typedef struct (\w+ )?\{(.*)\} ?(\w+)", decl)
        if m:
            body, name = m.group(2).strip(), m.group(3)
            if "{" in body or not body.endswith(";"):
                raise AbiError(f"include/ivit.h: cannot parse `{decl[:80]}`")
            abi.structs[name] = [d for member in body[:-1].split(";") for d in _declarators(member.strip(), abi, f"member of {name}")]
            continue
        m = re.fullmatch(r"enum \{(.*)\}", decl)
        if m:
            for item in m.group(1).split(","):
                e = re.fullmatch(r" ?(\w+) ?= ?(-?\d+) ?", item)
                if not e:
                    raise AbiError(f"include/ivit.h: enumerator `{item.strip()}` has no explicit integer value")
                abi.constants[e.group(1)] = int(e.group(2))
            continue
        if "{" in decl or decl.split(" ")[0] in ("typedef", "struct", "union", "enum"):
            raise AbiError(f"include/ivit.h: cannot parse declaration `{decl[:80]}`")
        fn = _function(decl, abi)
        abi.functions[fn.ret.name] = fn
    return abi


def ctype(d, structures, abi, ret=False):
    """the mapping rule of the module's docstring, for one parameter, field or return type"""
    if d.ptr or d.base in abi.handles:
        return ctypes.c_char_p if ret and d.type == "const char *" else ctypes.c_void_p
    return structures[d.base] if d.base in structures else SCALARS[d.base]


def structures(abi, names=None):
    """header name -> generated ctypes.Structure (class name: names[header name], else the header name)"""
    out = {}
    for name, fields in abi.structs.items():
        ft = [(d.name, ctype(d, out, abi) * d.array if d.array else ctype(d, out, abi)) for d in fields]
        out[name] = type((names or {}).get(name, name), (ctypes.Structure,), {"_fields_": ft, "__doc__": f"struct {name} (include/ivit.h)"})
    return out


def signatures(abi, structs):
    """name -> (restype, argtypes) of every prototype; an array parameter is the pointer it decays to"""
    return {name: (ctype(fn.ret, structs, abi, ret=True), [ctypes.c_void_p if p.array else ctype(p, structs, abi) for p in fn.params])
            for name, fn in abi.functions.items()}


with open(HEADER) as _f:
    ABI = parse(_f.read())
with open(EVAL_HEADER) as _f:
    EVAL_ABI = parse(_f.read(), base=ABI)
with open(FEATURES_HEADER) as _f:
    FEATURES_ABI = parse(_f.read(), base=ABI)
with open(ATTNMAP_HEADER) as _f:
    ATTNMAP_ABI = parse(_f.read(), base=ABI)
with open(CLASSMAP_HEADER) as _f:
    CLASSMAP_ABI = parse(_f.read(), base=ABI)
with open(HIDDEN_HEADER) as _f:
    HIDDEN_ABI = parse(_f.read(), base=ABI)
with open(SEARCH_HEADER) as _f:
    SEARCH_ABI = parse(_f.read(), base=ABI)
with open(MODELFILE_HEADER) as _f:
    MODELFILE_ABI = parse(_f.read(), base=ABI)
with open(PROBE_HEADER) as _f:
    PROBE_ABI = parse(_f.read(), base=ABI)
with open(VIEWS_HEADER) as _f:
    VIEWS_ABI = parse(_f.read(), base=ABI)
with open(CLUSTER_HEADER) as _f:
    CLUSTER_ABI = parse(_f.read(), base=ABI)
with open(RANGE_HEADER) as _f:
    RANGE_ABI = parse(_f.read(), base=ABI)
with open(JPEG_HEADER) as _f:
    JPEG_ABI = parse(_f.read(), base=ABI)
