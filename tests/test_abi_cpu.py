"""The one check of the Python/C boundary: masklab_hip/_lib.py against include/masklab_hip.h.

The header is parsed once (comments stripped).  Every prototype is held to its row of `_lib.SIGNATURES` type by type,
every struct to its mirror in `_lib.STRUCTS` field by field, every upper-case integer `X` of `_lib` to `ML_X`; the
structs' sizes and offsets are asked of the C compiler; and the layout of ABI 7 itself is pinned in one table below.  A
new entry point needs a declaration, a SIGNATURES row and nothing here."""
import ctypes as C
import keyword
import os
import re
import shutil
import subprocess

import pytest

from masklab_hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "masklab_hip.h")

# sizeof and the offsets that were pinned by hand while the struct grew, as the compiler lays out ABI 7
ABI7_LAYOUT = {
    "ml_conv2d_desc": (184, {"math": 144, "out_bstride": 152, "live": 160, "live_period": 168, "gn_partials": 176}),
    "ml_conv2d_wgrad_desc": (216, {}),
    "ml_dwconv3x3_grad_desc": (128, {}),
    "ml_deconv_out_problem": (96, {"live": 88}),
    "ml_deconv_out_grad_problem": (88, {}),
    "ml_gn_desc": (104, {"live": 72, "partials": 88, "n_partials": 96}),
    "ml_gn_grad_desc": (96, {"HWC": 64}),
    "ml_se_desc": (72, {"ws_offset": 64}),
    "ml_se_residual_desc": (104, {}),
    "ml_se_bottleneck_desc": (72, {}),
    "ml_roi_grad_level": (40, {}),
    "ml_opt_tensor": (48, {"n": 32}),
    "ml_opt_state": (16, {"lr": 8}),
    "ml_opt_scalars": (48, {"rectified": 40}),
    "ml_repack_job": (208, {"kind": 40, "first_unit": 200}),
}
LAYOUT_CHANGED = ("the layout of ABI 7 changed: bump ML_ABI_VERSION (header and _lib.ABI_VERSION) and pin the new "
                  "layout in a new table")

SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
           "uint8_t": C.c_uint8}


class Header:
    """functions: name -> (return type, [(type, parameter name)]); structs: name -> [(type, field name)];
    constants: ML_* name -> int.  A type is (base, pointer depth).  unreadable: every top-level declaration, field,
    parameter or ML_* macro that is none of the forms this parser knows -- the tests want it empty."""

    def __init__(self, text):
        self.functions, self.structs, self.constants, self.unreadable = {}, {}, {}, []
        self.text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        assert "//" not in self.text and "\\\n" not in self.text, "the header is C89-commented, one line per directive"
        body = []
        for line in self.text.splitlines():
            if line.lstrip().startswith("#"):
                self._directive(line.split())
            else:
                body.append(line)
        body = "\n".join(body)
        body, n = re.subn(r'extern\s+"C"\s*\{(.*)\}', r"\1", body, flags=re.S)      # the __cplusplus guard's braces
        assert n == 1, 'expected one extern "C" block'
        depth, start = 0, 0
        for i, ch in enumerate(body):                                                # statements end at a top-level ';'
            depth += (ch == "{") - (ch == "}")
            if ch == ";" and depth == 0:
                self._statement(" ".join(body[start:i].split()))
                start = i + 1
        if body[start:].strip():
            self.unreadable.append(body[start:].strip())

    def _directive(self, words):
        if words[0] == "#define" and words[1].startswith("ML_"):
            value = re.fullmatch(r"\(?(-?\d+)\)?", " ".join(words[2:]))
            if value:
                self.constants[words[1]] = int(value.group(1))
            else:
                self.unreadable.append(" ".join(words))
        elif words[0] not in ("#ifndef", "#ifdef", "#endif", "#include") and words[:2] != ["#define", "MASKLAB_HIP_H"]:
            self.unreadable.append(" ".join(words))

    def _statement(self, text):
        enum = re.fullmatch(r"enum \{(.*)\}", text)
        struct = re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", text)
        function = re.fullmatch(r"([\w\s\*]+?)\b(ml_\w+) ?\((.*)\)", text)
        if enum:
            value = -1
            for item in enum.group(1).split(","):
                m = re.fullmatch(r"\s*(ML_\w+)\s*(?:=\s*(-?\d+))?\s*", item)
                if not m:
                    return self.unreadable.append(f"enumerator `{item.strip()}`")
                value = int(m.group(2)) if m.group(2) else value + 1
                self.constants[m.group(1)] = value
        elif struct and struct.group(1) == struct.group(3):
            fields = []
            for decl in filter(None, (d.strip() for d in struct.group(2).split(";"))):
                base, declarators = re.fullmatch(r"((?:const )?\w*)\s*(.*)", decl).groups()    # `const float *x, *wd`
                for declarator in declarators.split(","):
                    m = re.fullmatch(r"\s*(\**)\s*(\w+)\s*", declarator)
                    ctype = self._type(base, m.group(1)) if m else None
                    if not m or ctype is None:
                        return self.unreadable.append(f"{struct.group(1)}: field `{decl}`")
                    fields.append((ctype, m.group(2)))
            self.structs[struct.group(1)] = fields
        elif function:
            params = []
            if function.group(3).strip() != "void":
                for p in function.group(3).split(","):
                    m = re.fullmatch(r"\s*([\w\s]+?)\s*((?:\*\s*(?:const\s*)?)*)(\w+)\s*(\[\w*\])?\s*", p)
                    ctype = self._type(m.group(1), m.group(2) + ("*" if m.group(4) else "")) if m else None      # `x[6]` = `*x`
                    if ctype is None:
                        return self.unreadable.append(f"{function.group(2)}: parameter `{p.strip()}`")
                    params.append((ctype, m.group(3)))
            ret = re.fullmatch(r"([\w\s]+?)\s*(\**)\s*", function.group(1))
            ret = self._type(ret.group(1), ret.group(2)) if ret else None
            if ret is None:
                return self.unreadable.append(f"{function.group(2)}: return type `{function.group(1).strip()}`")
            self.functions[function.group(2)] = (ret, params)
        else:
            self.unreadable.append(text)

    def _type(self, base, stars):
        """(base, depth) of `const`-stripped `base` followed by `stars`, or None for a base this parser does not know
        (a struct must be declared above its first use, as C wants it)."""
        words = [w for w in base.split() if w != "const"]
        if len(words) != 1 or not (words[0] in SCALARS or words[0] in ("void", "char") or words[0] in self.structs):
            return None
        return words[0], stars.count("*")


def c_name(ctype):
    return ctype[0] + " " + "*" * ctype[1] if ctype[1] else ctype[0]


def py_name(t):
    if t is None or isinstance(getattr(t, "_type_", ""), str):                       # simple types carry a format character
        return {None: "None", C.c_int32: "c_int32", C.c_int64: "c_int64"}.get(t, getattr(t, "__name__", ""))
    return f"POINTER({py_name(t._type_)})"


def bindings_of(header, ctype, where):
    """The ctypes types that may bind C type `ctype` as a parameter (`where` = "param"), a return value ("return") or
    a struct field ("field"); the first is the one to write."""
    base, depth = ctype
    if depth == 0:
        if base in header.structs:
            return [_lib.STRUCTS.get(base)] if where == "field" else []         # by value: fields only
        return [SCALARS[base]] if base in SCALARS and base != "uint8_t" else []
    if where == "return":
        return [C.c_char_p] if ctype == ("char", 1) else []
    if where == "field":
        return [C.c_void_p]
    if base in header.structs and depth == 1:
        return [C.POINTER(_lib.STRUCTS[base])] if base in _lib.STRUCTS else []
    pointee = C.c_void_p if depth > 1 else SCALARS.get(base)
    return [C.c_void_p] + ([C.POINTER(pointee)] if pointee else [])


@pytest.fixture(scope="module")
def header():
    with open(HEADER) as f:
        return Header(f.read())


def test_every_declaration_of_the_header_is_understood(header):
    """No silent gaps: what the parser read is what two loose regular expressions find, and nothing was left unread."""
    assert not header.unreadable, "declarations of masklab_hip.h this test cannot read:\n" + "\n".join(header.unreadable)
    declared = set(re.findall(r"\b(ml_[a-z0-9_]+)\s*\(", header.text))
    assert len(declared) >= 20
    assert set(header.functions) == declared, f"prototypes the parser missed: {sorted(declared ^ set(header.functions))}"
    structs = set(re.findall(r"typedef\s+struct\b[^;{]*\{[^}]*\}\s*(ml_\w+)\s*;", header.text))
    assert len(structs) >= 15
    assert set(header.structs) == structs, f"structs the parser missed: {sorted(structs ^ set(header.structs))}"
    macros = set(re.findall(r"^\s*#\s*define\s+(ML_\w+)", header.text, flags=re.M))
    assert macros <= set(header.constants), f"macros the parser missed: {sorted(macros - set(header.constants))}"


def test_every_prototype_is_bound_with_its_types_and_exported(header):
    assert set(_lib.SIGNATURES) == set(header.functions), (
        f"declared in masklab_hip.h without a row in _lib.SIGNATURES: {sorted(set(header.functions) - set(_lib.SIGNATURES))}; "
        f"rows without a declaration: {sorted(set(_lib.SIGNATURES) - set(header.functions))}")
    lib = C.CDLL(_lib.LIB_PATH)
    wrong = []
    for name, (ret, params) in header.functions.items():
        restype, argtypes = _lib.SIGNATURES[name]
        if not hasattr(lib, name):
            wrong.append(f"{name}: declared in masklab_hip.h but not exported by {os.path.basename(_lib.LIB_PATH)}")
        if restype not in bindings_of(header, ret, "return"):
            wrong.append(f"{name}: returns `{c_name(ret)}`, bound as {py_name(restype)}")
        if len(argtypes) != len(params):
            wrong.append(f"{name}: {len(params)} parameters declared, {len(argtypes)} bound")
            continue
        for i, ((ctype, pname), bound) in enumerate(zip(params, argtypes)):
            allowed = bindings_of(header, ctype, "param")
            if bound not in allowed:
                wrong.append(f"{name}: argument {i} is `{c_name(ctype)} {pname}`, bound as {py_name(bound)} "
                             f"(wants {' or '.join(map(py_name, allowed)) or 'a type this test knows'})")
    assert not wrong, "\n".join(wrong)


def test_every_struct_has_a_mirror_with_its_fields(header):
    assert set(_lib.STRUCTS) == set(header.structs), sorted(set(_lib.STRUCTS) ^ set(header.structs))
    wrong = []
    for name, fields in header.structs.items():
        mirror = _lib.STRUCTS[name]
        want = [f + "_" if keyword.iskeyword(f) else f for _, f in fields]
        got = [f for f, _ in mirror._fields_]
        if got != want:
            i = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
            wrong.append(f"{name}: field {i} is `{(want + ['(none)'])[i]}`, {mirror.__name__} has `{(got + ['(none)'])[i]}` "
                         f"({len(want)} fields declared, {len(got)} mirrored)")
            continue
        for (ctype, fname), (_, bound) in zip(fields, mirror._fields_):
            allowed = bindings_of(header, ctype, "field")
            if bound not in allowed:
                wrong.append(f"{name}.{fname}: `{c_name(ctype)}`, {mirror.__name__} has {py_name(bound)} "
                             f"(wants {' or '.join(map(py_name, allowed)) or 'a type this test knows'})")
    assert not wrong, "\n".join(wrong)


def host_c_compiler():
    """`cc`, else the clang beside the hipcc the Makefile builds with."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    beside = os.path.dirname(os.path.realpath(hipcc))
    for cc in (shutil.which("cc"), os.path.join(beside, "clang"), os.path.join(beside, "..", "lib", "llvm", "bin", "clang")):
        if cc and os.path.exists(cc):
            return cc
    return None


@pytest.fixture(scope="module")
def compiled_layout(header, tmp_path_factory):
    """struct -> (sizeof, {field: offsetof}) as the host C compiler lays out the header's structs."""
    cc = host_c_compiler()
    assert cc, "no host C compiler (neither `cc` nor a clang beside hipcc): the struct layouts cannot be checked"
    tmp = tmp_path_factory.mktemp("abi")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "masklab_hip.h"', 'int main(void) {']
    for name, fields in header.structs.items():
        lines.append(f'    printf("{name} . %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for _, f in fields]
    lines += ['    return 0;', '}']
    (tmp / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.dirname(HEADER), "-o", str(tmp / "layout"), str(tmp / "layout.c")], check=True)
    out = subprocess.run([str(tmp / "layout")], check=True, capture_output=True, text=True).stdout
    layout = {name: [None, {}] for name in header.structs}
    for name, field, value in (line.split() for line in out.splitlines()):
        if field == ".":
            layout[name][0] = int(value)
        else:
            layout[name][1][field] = int(value)
    return layout


def test_every_mirror_has_the_layout_the_c_compiler_gives_the_struct(compiled_layout):
    wrong = []
    for name, (size, offsets) in compiled_layout.items():
        mirror = _lib.STRUCTS[name]
        if C.sizeof(mirror) != size:
            wrong.append(f"sizeof({name}) = {size}, sizeof({mirror.__name__}) = {C.sizeof(mirror)}")
        for (field, _), (cfield, offset) in zip(mirror._fields_, offsets.items()):
            mine = getattr(mirror, field).offset
            if mine != offset:
                wrong.append(f"offsetof({name}, {cfield}) = {offset}, {mirror.__name__}.{field}.offset = {mine}")
    assert not wrong, "\n".join(wrong)


def test_abi_7_layout_is_the_pinned_one(header, compiled_layout):
    """Header and mirror agreeing is not enough: a library built from another layout would still load as version 7."""
    assert _lib.ABI_VERSION == 7 and set(ABI7_LAYOUT) == set(header.structs), LAYOUT_CHANGED
    for name, (size, offsets) in ABI7_LAYOUT.items():
        got_size, got_offsets = compiled_layout[name]
        assert got_size == size, f"sizeof({name}) is {got_size}, ABI 7 has {size}: {LAYOUT_CHANGED}"
        for field, offset in offsets.items():
            got = got_offsets.get(field)
            assert got == offset, f"offsetof({name}, {field}) is {got}, ABI 7 has {offset}: {LAYOUT_CHANGED}"


def test_every_constant_of_the_binding_is_the_headers(header):
    names = [n for n, v in vars(_lib).items() if n.isupper() and isinstance(v, int) and not isinstance(v, bool)]
    assert "ABI_VERSION" in names and len(names) >= 35
    wrong = []
    for n in names:
        if "ML_" + n not in header.constants:
            wrong.append(f"_lib.{n} = {getattr(_lib, n)}: masklab_hip.h has no ML_{n}")
        elif header.constants["ML_" + n] != getattr(_lib, n):
            wrong.append(f"_lib.{n} = {getattr(_lib, n)}, masklab_hip.h has ML_{n} = {header.constants['ML_' + n]}")
    assert not wrong, "\n".join(wrong)
