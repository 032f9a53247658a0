"""Reader of the C declarations include/lanefront.h is written in: integer constants (#define and enum), structs as
ctypes.Structure classes, opaque types and the prototypes behind an API marker.  A subset of C, on purpose: whatever is outside
it -- an unknown type, a function pointer, a union, a struct passed by value -- raises CDeclError naming the declaration.
Nothing ever defaults to int."""
import collections
import ctypes
import re

SCALARS = {
    "char": ctypes.c_char, "signed char": ctypes.c_byte, "unsigned char": ctypes.c_ubyte, "short": ctypes.c_short,
    "unsigned short": ctypes.c_ushort, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint,
    "long": ctypes.c_long, "unsigned long": ctypes.c_ulong, "long long": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
    "int8_t": ctypes.c_int8, "uint8_t": ctypes.c_uint8, "int16_t": ctypes.c_int16, "uint16_t": ctypes.c_uint16,
    "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
}
_NAME_DIMS = r"(\w+)((?:\s*\[\s*\w*\s*\])*)"
_DECLARATOR = re.compile(r"^(.*?)" + _NAME_DIMS + r"$", re.S)

# name, restype, argtypes and params (the parameter names) of one prototype; argtypes follow the typing rule of `Header`
Function = collections.namedtuple("Function", "name restype argtypes params")


class CDeclError(ValueError):
    pass


def camel(c_name):
    """lf_foo_bar -> LfFooBar"""
    return "".join(w.capitalize() for w in c_name.split("_"))


class Header(object):
    """What `text` declares: constants {name: int}, structs {C name: ctypes.Structure subclass named camel(C name)} in
    declaration order, opaque (the names of types declared without a body) and functions {name: Function} for the prototypes that
    start with `api`.  Typing rule: scalars by their C type; a pointer field, and a pointer parameter to an opaque type, a scalar,
    void or another pointer, is an address (c_void_p); a pointer parameter to a struct with a body is POINTER(its class); an array
    parameter is a pointer; a void return is None and a `const char*` return c_char_p.  base: the Header of a header that `text`
    includes: its structs, opaque types and constants may be named here, and stay its own."""

    def __init__(self, text, api="LF_API", base=None):
        self.api, self.constants, self.structs, self.opaque, self.functions = api, {}, {}, [], {}
        self.base = base
        statements = self._statements(self._preprocess(text))
        prototypes = [s for s in statements if s.startswith(api + " ")]
        for s in statements:                 # types first: a prototype may name a struct that is defined after it
            if s not in prototypes:
                self._type_declaration(s)
        self.opaque = [n for n in self.opaque if n not in self.structs]
        for s in prototypes:
            self._prototype(s)

    def _int(self, word, where):
        word = word.strip()
        if word in self.constants:
            return self.constants[word]
        if self.base is not None and word in self.base.constants:
            return self.base.constants[word]
        m = re.match(r"^\(?\s*(-?\s*(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]*\s*\)?$", word)
        if not m:
            raise CDeclError("not an integer constant: %r in `%s`" % (word, where))
        return int(m.group(1).replace(" ", ""), 0)

    def _preprocess(self, text):
        """comments and directives out; #define NAME <integer> into constants; #ifdef / #ifndef of names defined so far"""
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).replace("\\\n", " ")
        defined, skipping, kept = set(), [], []
        for line in text.split("\n"):
            m = re.match(r"^\s*#\s*(\w+)\s*(\w*)\s*(.*?)\s*$", line)
            if not m:
                if not any(skipping):
                    kept.append(line)
                continue
            directive, name, value = m.groups()
            if directive in ("ifdef", "ifndef"):
                skipping.append((name in defined) == (directive == "ifndef"))
            elif directive == "endif" and skipping:
                skipping.pop()
            elif directive == "define" and name:
                if not any(skipping):
                    defined.add(name)
                    if value and name != self.api:
                        self.constants[name] = self._int(value, line.strip())
            elif directive != "include":
                raise CDeclError("unsupported directive: `%s`" % line.strip())
        return "\n".join(kept)

    @staticmethod
    def _statements(text):
        """the text cut at the semicolons outside braces, whitespace collapsed"""
        out, depth, start = [], 0, 0
        for m in re.finditer(r"[{};]", text):
            depth += (m.group() == "{") - (m.group() == "}")
            if m.group() == ";" and depth == 0:
                out.append(" ".join(text[start:m.start()].split()))
                start = m.end()
        if depth != 0 or text[start:].strip():
            raise CDeclError("unterminated declaration: `%s`" % " ".join(text[start:].split())[:80])
        return [s for s in out if s]

    def _type_declaration(self, s):
        m = re.match(r"^(typedef )?(enum|struct)( \w+)? ?(?:\{(.*)\})? ?(\w+)?$", s)
        if not m:
            raise CDeclError("unsupported declaration: `%s`" % s[:120])
        typedef, kind, tag, body, alias = m.groups()
        tag = tag and tag.strip()
        if bool(typedef) != bool(alias) or (tag and alias and tag != alias) or not (tag or alias or kind == "enum"):
            raise CDeclError("unsupported declaration: `%s`" % s[:120])
        if kind == "enum":
            if body is None:
                raise CDeclError("enum without a body: `%s`" % s)
            value = -1
            for item in filter(None, (t.strip() for t in body.split(","))):
                name, _, expr = item.partition("=")
                value = self._int(expr, s[:120]) if expr else value + 1
                self.constants[name.strip()] = value
        elif body is None:
            self.opaque.append(alias or tag)         # `struct x;` before its definition is dropped from the list at the end
        else:
            self.structs[alias or tag] = self._struct(alias or tag, body, s)

    def _dims(self, dims, where):
        return [self._int(d, where) for d in re.findall(r"\[\s*(\w*)\s*\]", dims)]

    def _base(self, words, where):
        """(scalar ctypes type or None, struct class or None) of a type name without its stars; void, opaque -> (None, None)"""
        words = [w for w in words.split() if w != "const"]
        if words[:1] == ["struct"] and len(words) == 2:
            words = words[1:]
        name = " ".join(words)
        if name in SCALARS:
            return SCALARS[name], None
        if name in self.structs:
            return None, self.structs[name]
        if name == "void" or name in self.opaque:
            return None, None
        if self.base is not None:
            return self.base._base(name, where)
        raise CDeclError("unknown type %r in `%s`" % (name, where))

    def _struct(self, c_name, body, where):
        fields = []
        if "{" in body:
            raise CDeclError("nested definition in `%s`" % where[:120])
        for member in filter(None, (t.strip() for t in body.split(";"))):
            first, *more = member.split(",")
            m = _DECLARATOR.match(first.strip())
            others = [re.match(r"^\s*" + _NAME_DIMS + r"\s*$", d) for d in more]
            if not m or not m.group(1).strip() or not all(others) or ":" in member or "(" in member:
                raise CDeclError("unsupported member `%s` of %s" % (member, c_name))
            stars = m.group(1).count("*")
            scalar, struct = self._base(m.group(1).replace("*", " "), "%s in %s" % (member, c_name))
            if stars and more:
                raise CDeclError("several pointer declarators in `%s` of %s" % (member, c_name))
            if not stars and not (scalar or struct):
                raise CDeclError("member `%s` of %s has an incomplete type" % (member, c_name))
            for d in [m] + others:
                t = ctypes.c_void_p if stars else (scalar or struct)
                for n in reversed(self._dims(d.group(d.lastindex), member)):
                    t = t * n
                fields.append((d.group(d.lastindex - 1), t))
        return type(camel(c_name), (ctypes.Structure,), {"_fields_": fields, "__doc__": "`%s` of the header" % c_name})

    def _prototype(self, s):
        m = re.match(r"^%s (.*?)(\w+) ?\((.*)\)$" % re.escape(self.api), s)
        if not m or "(" in m.group(3) or not m.group(1).strip():
            raise CDeclError("unsupported prototype: `%s`" % s[:120])
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret.replace(" ", "") == "constchar*":
            restype = ctypes.c_char_p
        elif "*" in ret:
            self._base(ret.replace("*", " "), s[:120])
            restype = ctypes.c_void_p
        else:
            restype = self._base(ret, s[:120])[0]
            if restype is None and ret != "void":
                raise CDeclError("%s returns %r by value" % (name, ret))
        argtypes, names = [], []
        for p in ([] if params == "void" else params.split(",")):
            d = _DECLARATOR.match(p.strip())
            if not d or not d.group(1).strip():
                raise CDeclError("unsupported parameter `%s` of %s" % (p.strip(), name))
            depth = d.group(1).count("*") + (1 if d.group(3).strip() else 0)
            scalar, struct = self._base(d.group(1).replace("*", " "), "%s of %s" % (p.strip(), name))
            if depth == 0 and scalar is None:
                raise CDeclError("parameter `%s` of %s is not a scalar or a pointer" % (p.strip(), name))
            argtypes.append(scalar if depth == 0 else ctypes.POINTER(struct) if depth == 1 and struct else ctypes.c_void_p)
            names.append(d.group(2))
        if name in self.functions:
            raise CDeclError("%s is declared twice" % name)
        self.functions[name] = Function(name, restype, argtypes, names)
