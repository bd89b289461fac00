"""The ctypes declarations of the C ABI, made from include/mtadgat.h itself: the header is the one place an entry point is
written down, and Header.bind() sets argtypes and restype of every prototype it holds on the loaded library.

The parser reads the `#define MTADGAT_* <int>` constants, the `typedef struct { ... }` field lists and every `mtadgat_*`
prototype, comments stripped (those inside parameter lists too).  How a parameter maps:
  - a scalar by its width; `const char*` is c_char_p; mtadgat_handle is c_void_p and `mtadgat_handle*` POINTER(c_void_p);
  - a pointer to a struct of the header: POINTER(the ctypes.Structure registered for it), or c_void_p when the parameter is
    named *_dev (the records live in device memory);
  - a pointer to a scalar named *_host, and an array declarator (`double ms[N]`): POINTER(that scalar) -- host memory;
  - every other pointer to a scalar or to void: c_void_p.  tests/pointer_proxy.py holds exactly these to the arena as device
    pointers, so the header's *_dev / *_host naming is what separates the two.
Anything else raises ValueError quoting the prototype: nothing is left to ctypes' defaults, the restype c_int included.
"""
import ctypes
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "mtadgat.h")

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
           "uint8_t": ctypes.c_uint8, "unsigned char": ctypes.c_ubyte}
HANDLE = "mtadgat_handle"


class Header:
    """defines {name: int} and structs {name: [(field, ctype)]}, pointers as c_void_p and arrays as ctype * n, as soon as the text is
    read, so that the package can size its Structures by them; register() then takes those Structures and makes prototypes
    {name: (restype, [(parameter, ctype)], text)}."""

    def __init__(self, text):
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        self.defines = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MTADGAT_\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
        text = re.sub(r'^[ \t]*#[^\n]*$|extern\s+"C"\s*\{', " ", text, flags=re.M)
        self.structs, self.structures = {}, {}
        for body, name in re.findall(r"typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
            self.structs[name] = [f for decl in body.split(";") if decl.strip() for f in self._fields(decl, name)]
        text = re.sub(r"typedef\s+(struct|enum)\s+\w*\s*\{[^{}]*\}\s*\w+\s*;", " ", text)
        self._statements = [" ".join(stmt.split()) for stmt in text.split(";")]

    def register(self, **structures):
        """structures: {struct name: the ctypes.Structure that mirrors it}, checked field by field."""
        for name, cls in structures.items():
            if list(cls._fields_) != self.structs[name]:
                raise ValueError(f"{cls.__name__} does not mirror {name} of include/mtadgat.h")
        self.structures, self.prototypes = structures, {}
        for stmt in self._statements:
            if stmt in ("", "}") or re.fullmatch(r"typedef struct \w+ ?\* ?" + HANDLE, stmt):
                continue
            m = re.fullmatch(r"(.+?)\b(mtadgat_\w+) ?\(([^()]*)\)", stmt)
            if not m:
                raise ValueError(f"not a prototype the binder can read: `{stmt}`")
            restype = self._parameter(m.group(1) + " result", stmt)[1]
            params = [] if m.group(3).strip() in ("", "void") else [self._parameter(p, stmt) for p in m.group(3).split(",")]
            self.prototypes[m.group(2)] = (restype, params, stmt)
        return self

    @staticmethod
    def _split(decl, where):
        """(base type, pointer depth, name, array bound or None) of a declarator such as `const T* name[N]`."""
        m = re.fullmatch(r"\s*(.*?)(\w+)\s*(?:\[\s*(\w*)\s*\])?\s*", decl, re.S)
        words = m.group(1).replace("*", " * ").split() if m else []
        base = " ".join(w for w in words if w not in ("const", "*"))
        if not base:
            raise ValueError(f"cannot read the declarator `{decl.strip()}` of `{where}`")
        return base, words.count("*"), m.group(2), m.group(3)

    def _fields(self, decl, where):
        pieces = decl.split(",")                                  # `float lo, hi, scale;`: the declarators share the base type
        base = self._split(pieces[0], where)[0]
        for i, piece in enumerate(pieces):
            _, stars, name, bound = self._split(piece if i == 0 else base + " " + piece, where)
            t = ctypes.c_void_p if stars else self._ctype(base, 0, name, None, where)
            yield name, (t if bound is None else t * (self.defines.get(bound) or int(bound)))

    def _parameter(self, decl, where):
        base, stars, name, bound = self._split(decl, where)
        return name, self._ctype(base, stars, name, bound, where)

    def _ctype(self, base, stars, name, bound, where):
        scalar, t = SCALARS.get(base), None
        if bound is not None:
            t = ctypes.POINTER(scalar) if scalar and stars == 0 else None
        elif stars == 0:
            t = ctypes.c_void_p if base == HANDLE else scalar
        elif base == "char":
            t = ctypes.c_char_p if stars == 1 else None
        elif base == HANDLE:
            t = ctypes.POINTER(ctypes.c_void_p) if stars == 1 else None
        elif base in self.structs:
            if stars == 1 and base in self.structures:
                t = ctypes.POINTER(self.structures[base])
            elif stars == 1 and name.endswith("_dev"):
                t = ctypes.c_void_p
        elif scalar or base == "void":
            t = ctypes.POINTER(scalar) if scalar and stars == 1 and name.endswith("_host") else ctypes.c_void_p
        if t is None:
            raise ValueError(f"the binder does not know the type `{base}{'*' * stars}` of `{name}` in `{where}`")
        return t

    def bind(self, lib):
        """argtypes and restype of every prototype onto `lib`."""
        for name, (restype, params, _) in self.prototypes.items():
            fn = getattr(lib, name)
            fn.argtypes = [t for _, t in params]
            fn.restype = restype
        return lib


def read(path=HEADER_PATH):
    with open(path) as f:
        return Header(f.read())
