"""Reads the restricted C of include/strongsort_hip.h into ctypes: integer `#define`s, `typedef struct` blocks of scalars and
pointers, flat function declarations.  lib.py binds the library from the result, so a signature is written once, in the header.
Text that fits none of these forms raises HeaderError: nothing is guessed, nothing is skipped.

Pointers:  const char*, const unsigned char* -> c_char_p (host bytes);  a name starting with d_ (device memory), void*, ss_ctx*
and the raw output buffers unsigned char* / unsigned int* -> c_void_p (callers pass addresses);  T** and T* const* ->
POINTER(what T* maps to);  any other T* -> POINTER(T), so a host array of the wrong type is a ctypes.ArgumentError.
"""
import ctypes as C
import re

SCALARS = {"char": C.c_char, "unsigned char": C.c_ubyte, "short": C.c_short, "unsigned short": C.c_ushort, "int": C.c_int,
           "unsigned": C.c_uint, "unsigned int": C.c_uint, "long long": C.c_longlong, "size_t": C.c_size_t, "float": C.c_float,
           "double": C.c_double, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}


class HeaderError(ValueError):
    pass


class Header:
    """defines: name -> int;  structs: name -> ctypes.Structure subclass;  opaque: names of `typedef struct X X;`;
    functions: name -> (restype, [argtypes]) in declaration order."""

    def __init__(self, text):
        self.defines, self.structs, self.opaque, self.functions = {}, {}, set(), {}
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        code = []
        for line in text.splitlines():
            m = re.match(r"\s*#\s*define\s+(\w+)\s+(\S.*?)\s*$", line)
            if m:                                   # a #define with a value (the include guard has none)
                v = re.fullmatch(r"\(?\s*(-?\d+)\s*\)?", m.group(2))
                if not v:
                    raise HeaderError(f"#define {m.group(1)} is not an integer: {m.group(2)!r}")
                self.defines[m.group(1)] = int(v.group(1))
            elif not line.lstrip().startswith("#"):
                code.append(line)
        text = "\n".join(code).rstrip()
        m = re.search(r'extern\s+"C"\s*\{', text)
        if m:                                       # the block spans the rest of the header
            if not text.endswith("}"):
                raise HeaderError('extern "C" { is not closed at the end of the header')
            text = text[:m.start()] + text[m.end():-1]
        depth, start = 0, 0
        for i, ch in enumerate(text):
            depth += (ch == "{") - (ch == "}")
            if ch == ";" and depth == 0:
                self._statement(" ".join(text[start:i].split()))
                start = i + 1
        if text[start:].strip():
            raise HeaderError(f"unterminated declaration: {' '.join(text[start:].split())[:200]!r}")

    def _statement(self, s):
        opaque = re.fullmatch(r"typedef struct (\w+) \1", s)
        struct = re.fullmatch(r"typedef struct (\w+) \{([^{}]*)\} \1", s)
        func = re.fullmatch(r"([\w\s*]+?)\b(\w+) ?\(([^()]*)\)", s)
        if opaque:
            self.opaque.add(opaque.group(1))
        elif struct:
            fields = []
            for decl in filter(None, (d.strip() for d in struct.group(2).split(";"))):
                first, *more = decl.split(",")      # `int B, H, W`: the names after the first share its type
                ctype, name = self._declarator(first, s)
                if more and ("*" in decl or not all(re.fullmatch(r"\s*[A-Za-z_]\w*\s*", n) for n in more)):
                    raise HeaderError(f"cannot classify the field list {decl!r}")
                fields += [(name, ctype)] + [(n.strip(), ctype) for n in more]
            self.structs[struct.group(1)] = type(struct.group(1), (C.Structure,), {"_fields_": fields})
        elif func and func.group(2) not in self.functions:
            params = func.group(3).strip()
            args = [] if params == "void" else [self._declarator(p, s)[0] for p in params.split(",")]
            self.functions[func.group(2)] = (self._ctype(func.group(1), "", s, result=True), args)
        else:
            raise HeaderError(f"cannot classify: {s[:200]!r}")

    def _declarator(self, decl, where):
        m = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", decl)
        if not m:
            raise HeaderError(f"no `type name` in {decl.strip()!r}: {where[:200]!r}")
        return self._ctype(m.group(1), m.group(2), where), m.group(2)

    def _ctype(self, spec, name, where, result=False):
        tokens = re.findall(r"\w+|\S", spec)
        stars = tokens.count("*")
        words = tokens[:tokens.index("*")] if stars else tokens
        const, base = "const" in words, " ".join(w for w in words if w != "const")
        known = base in SCALARS or base in self.structs or base in self.opaque or base == "void"
        if not known or stars > 2 or any(t not in ("*", "const") for t in tokens[len(words):]):
            raise HeaderError(f"unknown type {spec.strip()!r} in {where[:200]!r}")
        if stars == 0 and base == "void" and result:
            return None
        if stars == 0 and base not in SCALARS:
            raise HeaderError(f"{base} by value in {where[:200]!r}")
        return self._map(base, const, stars, name)

    def _map(self, base, const, stars, name):
        if stars == 0:
            return SCALARS[base]
        if stars == 2:
            return C.POINTER(self._map(base, const, 1, ""))
        if const and base in ("char", "unsigned char"):
            return C.c_char_p
        if name.startswith("d_") or base == "void" or base in self.opaque or (not const and base in ("unsigned char", "unsigned int")):
            return C.c_void_p
        return C.POINTER(self.structs.get(base) or SCALARS[base])


def parse(path):
    with open(path) as f:
        return Header(f.read())
