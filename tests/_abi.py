"""include/wun.h read as data, and its comparison with the ctypes binding (wave_u_net_amd._lib), for tests/test_abi_host.py.

A type is None (void), a scalar (kind, bytes) with kind "int" / "uint" / "float" / "char", a struct's or the opaque plan's name,
or ("ptr", pointee).  parse() raises ValueError for anything in the header it does not understand; the compare_* functions return
the list of disagreements (empty = the binding is the header's)."""
import ctypes as C
import re

from wave_u_net_amd._lib import c_name

SCALARS = {"int": ("int", 4), "int32_t": ("int", 4), "int64_t": ("int", 8), "uint8_t": ("uint", 1), "uint32_t": ("uint", 4),
           "float": ("float", 4), "double": ("float", 8), "char": ("char", 1)}
_CODES = {"f": "float", "d": "float", "c": "char", "b": "int", "h": "int", "i": "int", "l": "int", "q": "int",
          "B": "uint", "H": "uint", "I": "uint", "L": "uint", "Q": "uint"}


def _type(text, names):
    """`const float*`, `void* const*`, `wun_plan**`, `int64_t` ... -> a type; `names`: the struct / opaque names declared so far."""
    words = re.sub(r"\bconst\b", " ", text).replace("*", " * ").split()
    if not words or words[0] == "*" or words[1:] != ["*"] * (len(words) - 1):
        raise ValueError("type not understood: %r" % text)
    if words[0] == "void":
        t = None
    elif words[0] in SCALARS:
        t = SCALARS[words[0]]
    elif words[0] in names:
        t = words[0]
    else:
        raise ValueError("unknown type %r in %r" % (words[0], text))
    for _ in range(len(words) - 1):
        t = ("ptr", t)
    return t


def _declarator(text):
    m = re.match(r"^(.*?)\b([A-Za-z_]\w*)\s*(?:\[\s*(\w+)\s*\])?$", text.strip())
    if not m:
        raise ValueError("declarator not understood: %r" % text)
    return m.group(1).strip(), m.group(2), m.group(3)


def _fields(body, names, defines):
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        first, *rest = decl.split(",")
        ctype, name, length = _declarator(first)
        for piece in [None] + rest:
            if piece is not None:
                more, name, length = _declarator(piece)
                if more:
                    raise ValueError("declarator not understood: %r in %r" % (piece, decl))
            if length is not None:
                length = int(length) if length.isdigit() else defines[length]       # KeyError: a length that is no #define
            fields.append((name, _type(ctype, names), length))
    return fields


def parse(path):
    """{"functions": {name: (return type, [argument types])}, "structs": {name: [(field, type, array length or None)]},
    "opaque": {names}, "defines": {name: int}, "enums": {name: int}}."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"#ifdef __cplusplus\n[^\n]*\n#endif", " ", text)         # extern "C" { ... }
    out = {"functions": {}, "structs": {}, "opaque": set(), "enums": {},
           "defines": {k: int(v) for k, v in re.findall(r"^[ \t]*#define[ \t]+(\w+)[ \t]+(\d+)u?[ \t]*$", text, re.M)}}
    for line in re.findall(r"^[ \t]*#.*$", text, re.M):
        w = line.split()
        known = w[0] in ("#ifndef", "#endif", "#include") or w == ["#define", "WUN_H"]
        if not known and (w[0] != "#define" or w[1] not in out["defines"]):
            raise ValueError("preprocessor line not understood: %r" % line)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    depth, start, statements = 0, 0, []
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            statements.append(" ".join(text[start:i].split()))
            start = i + 1
    if depth or text[start:].strip():
        raise ValueError("unterminated text at the end of the header: %r" % text[start:].strip()[:80])
    for st in statements:
        names = set(out["structs"]) | out["opaque"]
        m = re.match(r"^(?:typedef )?enum(?: \w+)? \{([^{}]*)\}(?: \w+)?$", st)
        if m:
            for item in m.group(1).split(","):
                if item.strip():
                    k, v = item.split("=")
                    out["enums"][k.strip()] = int(v)
            continue
        m = re.match(r"^typedef struct (\w+) (\w+)$", st)
        if m and m.group(1) == m.group(2):
            out["opaque"].add(m.group(2))
            continue
        m = re.match(r"^typedef struct(?: (\w+))? \{([^{}]*)\} (\w+)$", st)
        if m and m.group(1) in (None, m.group(3)) and m.group(3) not in names:
            out["structs"][m.group(3)] = _fields(m.group(2), names, out["defines"])
            continue
        m = re.match(r"^([\w\s\*]+?)\b(wun_\w+) ?\(([^()]*)\)$", st)
        if m and m.group(2) not in out["functions"]:
            args = [a.strip() for a in m.group(3).split(",")] if m.group(3).strip() != "void" else []
            types = []
            for a in args:
                ctype, name, length = _declarator(a)
                if length is not None:
                    raise ValueError("array parameter in %r" % st)
                types.append(_type(ctype if ctype else name, names))         # (an unnamed parameter is all type)
            out["functions"][m.group(2)] = (_type(m.group(1), names), types)
            continue
        raise ValueError("header statement not understood: %r" % st[:200])
    return out


def describe(ct):
    """A ctypes type of the binding in the parser's terms; c_void_p is ("ptr", "any")."""
    if ct is None:
        return None
    if ct is C.c_void_p:
        return ("ptr", "any")
    if ct is C.c_char_p:
        return ("ptr", ("char", 1))
    if issubclass(ct, C.Structure):
        return c_name(ct)
    if issubclass(ct, C._Pointer):
        return ("ptr", describe(ct._type_))
    if issubclass(ct, C._SimpleCData) and ct._type_ in _CODES:
        return (_CODES[ct._type_], C.sizeof(ct))
    raise ValueError("binding type not understood: %r" % (ct,))


def _mismatch(want, got):
    """Why the binding's type `got` does not serve the header's type `want`, or None."""
    wp, gp = isinstance(want, tuple) and want[0] == "ptr", isinstance(got, tuple) and got[0] == "ptr"
    if wp != gp:
        return "pointer in the header, scalar in the binding" if wp else "scalar in the header, pointer in the binding"
    if not wp:
        if want == got:
            return None
        if isinstance(want, tuple) and isinstance(got, tuple):
            return "kind %s != %s" % (want[0], got[0]) if want[0] != got[0] else "width %d != %d" % (want[1], got[1])
        return "%r != %r" % (want, got)
    if got[1] == "any":                                                       # c_void_p serves any pointer
        return None
    why = _mismatch(want[1], got[1])
    return None if why is None else "pointee: " + why


def compare_functions(functions, sigs):
    bad = ["%s: declared, not bound" % n for n in sorted(set(functions) - set(sigs))]
    bad += ["%s: bound, not declared" % n for n in sorted(set(sigs) - set(functions))]
    for name in sorted(set(functions) & set(sigs)):
        (ret, args), (res, argtypes) = functions[name], sigs[name]
        if ret != describe(res):
            bad.append("%s: return type %r != %r" % (name, ret, describe(res)))
        if len(args) != len(argtypes):
            bad.append("%s: arity %d != %d" % (name, len(args), len(argtypes)))
            continue
        for i, (want, got) in enumerate(zip(args, argtypes)):
            why = _mismatch(want, describe(got))
            if why:
                bad.append("%s: argument %d: %s" % (name, i, why))
    return bad


def compare_structs(structs, bound):
    """`bound`: the binding's Structure classes."""
    mine = {c_name(cls): cls for cls in bound}
    bad = ["%s: declared, not bound" % n for n in sorted(set(structs) - set(mine))]
    bad += ["%s: bound, not declared" % n for n in sorted(set(mine) - set(structs))]
    for name in sorted(set(structs) & set(mine)):
        want, got = structs[name], mine[name]._fields_
        if [f[0] for f in want] != [f[0] for f in got]:
            bad.append("%s: fields %s != %s" % (name, [f[0] for f in want], [f[0] for f in got]))
            continue
        for (field, ctype, length), (_, ct) in zip(want, got):
            is_array = isinstance(ct, type) and issubclass(ct, C.Array)
            if (length is not None) != is_array or (is_array and ct._length_ != length):
                bad.append("%s.%s: array length %r != %r" % (name, field, length, ct._length_ if is_array else None))
                continue
            why = _mismatch(ctype, describe(ct._type_ if is_array else ct))
            if why:
                bad.append("%s.%s: %s" % (name, field, why))
    return bad
