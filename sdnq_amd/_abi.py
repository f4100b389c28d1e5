"""Reader of ``include/sdnq_hip.h``: the ctypes side of the C ABI is derived from the header's declarations, not restated.

The header is regular C -- comments, preprocessor lines, ``typedef enum``, ``typedef struct`` and prototypes -- and this reads exactly
that.  It fails closed: a spelling outside the type table, a declarator it does not know or a ``sdnq_hip_x(`` that is not part of a
prototype it parsed raises SdnqHipError naming the header line.  It never guesses a type: a wrong ctypes row is no Python error, it is a
truncated pointer on the device.  tests/test_cabi.py hands everything read here back to the C compiler.
"""
import ctypes
import re


class SdnqHipError(RuntimeError):
    pass


# the type table: header spelling -> ctypes type
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double, "sdnq_stream_t": ctypes.c_void_p}
RETURNS = {**SCALARS, "void": None, "const char*": ctypes.c_char_p}
TYPED_POINTERS = ("const SdnqWeight*", "const SdnqLinearArgs*")  # POINTER(struct): ctypes' auto-byref and its rejection of another struct
# every other pointer spelling (parameters and fields) is an address: c_void_p

_SKIP = re.compile(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", re.S | re.M)  # comments and preprocessor lines
_ENUM = re.compile(r"typedef\s+enum\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;")
_PROTO = re.compile(r"^([\w \t*]+?)\b(sdnq_hip_\w+)\s*\(([^(){};]*)\)\s*;", re.M)  # a prototype starts its line
_TOKEN = re.compile(r"sdnq_hip_\w+\s*\(")
_DECL = re.compile(r"([\w\s*]*[\s*])(\w+)")  # "<type spelling> <name>"


def _spell(s: str) -> str:
    """One spelling per type: single spaces, every `*` attached to what is left of it."""
    return " ".join(s.replace("*", "* ").split()).replace(" *", "*")


class Header:
    """enums {SDNQ_NAME: value}; structs {name: [(field, spelling)]} and classes {name: ctypes.Structure}; prototypes
    [(return spelling, name, [parameter spellings])] and signatures {name: (restype, [argtypes])}, all in header order."""

    def __init__(self, text: str):
        self._text = text = _SKIP.sub(lambda m: "\n" * m.group().count("\n"), text)  # line numbers survive
        self.enums, self.structs, self.classes, self.prototypes, self.signatures = {}, {}, {}, [], {}
        for m in _ENUM.finditer(text):
            for item in re.finditer(r"[^,\s][^,]*", m.group(2)):
                kv = re.fullmatch(r"(SDNQ_\w+)\s*=\s*(-?\d+)\s*", item.group())
                if not kv:
                    self._fail(m.start(2) + item.start(), f"enum constant {item.group().strip()!r} without a literal value")
                self.enums[kv.group(1)] = int(kv.group(2))
        for m in _STRUCT.finditer(text):
            fields, ctypes_fields = [], []
            for d in re.finditer(r"[^;\s][^;]*", m.group(2)):
                at = m.start(2) + d.start()
                first, *more = (p.strip() for p in d.group().split(","))
                decl = _DECL.fullmatch(first)
                if not decl or not all(re.fullmatch(r"\w+", n) for n in more):
                    self._fail(at, f"field declarator {d.group().strip()!r} (arrays, bit-fields and pointer lists are not read)")
                spelling = _spell(decl.group(1))
                fields += [(n, spelling) for n in (decl.group(2), *more)]
                ctypes_fields += [(n, self.ctype(spelling, at)) for n in (decl.group(2), *more)]
            self.structs[m.group(1)] = fields
            self.classes[m.group(1)] = type(m.group(1), (ctypes.Structure,), {
                "__doc__": f"{m.group(1)} of include/sdnq_hip.h (fields in header order).", "_fields_": ctypes_fields})
        starts = set()
        for m in _PROTO.finditer(text):
            at, name, params = m.start(2), m.group(2), []
            ret = _spell(m.group(1))
            if m.group(3).strip() != "void":
                for p in m.group(3).split(","):
                    decl = _DECL.fullmatch(p.strip())
                    if not decl:
                        self._fail(at, f"parameter {p.strip()!r} of {name} is not `type name`")
                    params.append(_spell(decl.group(1)))
            starts.add(at)
            self.prototypes.append((ret, name, params))
            self.signatures[name] = (self.ctype(ret, at, returns=True), [self.ctype(p, at) for p in params])
        for t in _TOKEN.finditer(text):
            if t.start() not in starts:
                self._fail(t.start(), f"{t.group()!r} is not part of a prototype this reader understands")

    def ctype(self, spelling: str, at: int, returns: bool = False):
        table = RETURNS if returns else SCALARS
        if spelling in table:
            return table[spelling]
        if spelling.endswith("*") and not returns:
            if spelling not in TYPED_POINTERS:
                return ctypes.c_void_p
            if spelling[len("const "):-1] in self.classes:
                return ctypes.POINTER(self.classes[spelling[len("const "):-1]])
        self._fail(at, f"type {spelling!r} is not in the type table")

    def _fail(self, at: int, what: str):
        raise SdnqHipError(f"include/sdnq_hip.h line {self._text.count(chr(10), 0, at) + 1}: {what}")
