"""The ctypes binding is derived from include/mcgen_hip.h (mcgen_amd/_abi.py).  Checked here without a GPU: the reader on
small synthetic headers, its reading of the real header by a C++ compiler (layouts, signatures, constants), and the
number of arguments at every call site of an entry point."""
import ast
import ctypes as C
import glob
import os
import shutil
import subprocess

import pytest

from mcgen_amd import _lib
from mcgen_amd._abi import Header, HeaderError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYNTHETIC = '''
/* a comment with ; and ( and a fake int mcgen_foo(int x); in it */
#ifndef T_H
#define T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define T_MAX 16
#define T_HEX 0x20   /* trailing comment; with mcgen_bar( */
enum { T_A = 0, T_B = 1 };
enum { R_TILED = 0,    /* one ( */
       R_MC, R_GK, R_PP,     // a line comment; int mcgen_baz(void);
       R_JUMP = 10, R_NEXT };
typedef struct {
    const void*  x; const float* scale;      /* two declarations on a line */
    int32_t N, H, W;                         /* three declarators */
    const float *a, *b; float* c;
    int64_t big; double d; float f; int i;
    const int16_t* cmap;
} t_seg_t;
typedef struct { t_seg_t seg[2]; int32_t nseg; t_seg_t one; float alpha; } t_conv_t;
/* a comment that spans lines
int mcgen_hidden(int a);
*/
const char* t_last_error(void);
int t_version(void);      /* 9 (additions; without (a bump): t_adam(advance_step); 8: x */
int64_t t_elems(const t_conv_t* p, int dtype);
int32_t t_stride(int C);
int t_launch(const t_conv_t* p, const t_seg_t* table_dev, int n, float alpha, double count, int64_t pixels,
             const int64_t* label, int* out, t_seg_t* jobs, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* T_H */
'''


def test_reader_on_synthetic_header():
    h = Header(SYNTHETIC)
    assert h.constants == {'T_MAX': 16, 'T_HEX': 32, 'T_A': 0, 'T_B': 1, 'R_TILED': 0, 'R_MC': 1, 'R_GK': 2, 'R_PP': 3,
                           'R_JUMP': 10, 'R_NEXT': 11}
    seg, conv = h.structs['t_seg_t'], h.structs['t_conv_t']
    vp = C.c_void_p
    assert seg._fields_ == [('x', vp), ('scale', vp), ('N', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                            ('a', vp), ('b', vp), ('c', vp), ('big', C.c_int64), ('d', C.c_double), ('f', C.c_float),
                            ('i', C.c_int), ('cmap', vp)]
    assert [n for n, _ in conv._fields_] == ['seg', 'nseg', 'one', 'alpha']
    assert conv._fields_[0][1]._type_ is seg and conv._fields_[0][1]._length_ == 2 and conv._fields_[2][1] is seg
    assert C.sizeof(conv) == 3 * C.sizeof(seg) + 16 and conv.one.offset == 2 * C.sizeof(seg) + 8
    # prototypes: nothing from a comment, `void` lists are empty, returns keep their width
    assert list(h.functions) == ['t_last_error', 't_version', 't_elems', 't_stride', 't_launch']
    assert h.symbol('t_last_error') == (C.c_char_p, [])
    assert h.symbol('t_version') == (C.c_int, [])
    assert h.symbol('t_elems') == (C.c_int64, [C.POINTER(conv), C.c_int])
    assert h.symbol('t_stride') == (C.c_int32, [C.c_int])
    # struct pointers: host memory is typed, a name ending in _dev is a device address; other pointers are addresses
    assert h.symbol('t_launch') == (C.c_int, [C.POINTER(conv), vp, C.c_int, C.c_float, C.c_double, C.c_int64, vp, vp,
                                              C.POINTER(seg), vp])
    ret, params = h.functions['t_launch']
    assert [p.name for p in params] == ['p', 'table_dev', 'n', 'alpha', 'count', 'pixels', 'label', 'out', 'jobs', 'stream']
    assert params[6] == (True, 'int64_t', 1, 'label', None) and params[7] == (False, 'int', 1, 'out', None)
    assert h.fields['t_conv_t'][0] == (False, 't_seg_t', 0, 'seg', 2)


@pytest.mark.parametrize('text, naming', [
    ('int f(unsigned n);', 'unsigned'),                                   # a type the reader does not know
    ('typedef struct { int32_t a; uint8_t b; } s_t;', 'uint8_t'),
    ('typedef struct { int32_t a; } s_t; int f(const other_t* p);', 'other_t'),
    ('int f(void); static', 'static'),                                    # a stray token
    ('int f(void) { return 0; }', 'return'),
    ('#define T_F 1.5\n', '1.5'),
    ('#pragma once\nint f(void);', 'pragma'),
    ('int f(int (*cb)(int));', 'cb'),
    ('/* int mcgen_foo(int x); /* still the same comment */ int f(void); */', '*/'),   # C comments do not nest
    ('int f(void);\n/* never closed: int mcgen_foo(int x);', '/*'),
])
def test_reader_refuses_what_it_does_not_understand(text, naming):
    with pytest.raises(HeaderError) as e:
        Header(text)
    assert naming in str(e.value)


def _cxx():
    beside_hipcc = os.path.dirname(os.path.realpath(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')))
    for c in (os.environ.get('CXX'), 'c++', os.path.join(beside_hipcc, 'clang++'),
              os.path.join(beside_hipcc, '..', 'llvm', 'bin', 'clang++'), os.path.join(beside_hipcc, 'amdclang++')):
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError('no C++ compiler: set CXX')


def _render(d):
    return ('const ' if d.const else '') + d.base + '*' * d.depth


def abi_check_source(h: Header) -> str:
    """One C++17 translation unit of static_asserts: what ctypes will assume == what the compiler sees in the header."""
    out = ['#include <cstddef>', '#include <type_traits>', '#include "mcgen_hip.h"']
    for name, cls in h.structs.items():
        out.append(f'static_assert(sizeof({name}) == {C.sizeof(cls)}, "sizeof {name}");')
        for fname, _ in cls._fields_:
            f = getattr(cls, fname)
            out.append(f'static_assert(offsetof({name}, {fname}) == {f.offset} && sizeof({name}::{fname}) == {f.size}, '
                       f'"{name}.{fname}");')
    for name, (ret, params) in h.functions.items():
        out.append(f'static_assert(std::is_same_v<decltype(&{name}), {_render(ret)}(*)({", ".join(map(_render, params))})>, '
                   f'"{name}");')
        for i, (d, t) in enumerate(zip([ret] + params, [h.ctype(ret)] + h.symbol(name)[1])):     # the ctypes side of each
            fp = 'true' if t in (C.c_float, C.c_double) else 'false'
            out.append(f'static_assert(sizeof({_render(d)}) == {C.sizeof(t)} && std::is_floating_point_v<{_render(d)}> == {fp}, '
                       f'"{name} #{i}");')
    out += [f'static_assert({name} == {value}, "{name}");' for name, value in h.constants.items()]
    return '\n'.join(out) + '\n'


def compile_abi_check(h: Header, include_dir: str, tmp_path) -> subprocess.CompletedProcess:
    src = os.path.join(str(tmp_path), 'abi_check.cpp')
    with open(src, 'w') as f:
        f.write(abi_check_source(h))
    return subprocess.run([_cxx(), '-fsyntax-only', '-std=c++17', '-I', include_dir, src], capture_output=True, text=True)


def test_compiler_agrees_with_the_derived_binding(tmp_path):
    h = _lib.HEADER
    assert len(h.structs) >= 20 and len(h.functions) >= 123 and len(h.constants) >= 20
    assert h.constants['MCGEN_ROUTE_HEAD'] == 8 and C.sizeof(_lib.Conv) == 352
    r = compile_abi_check(h, os.path.join(ROOT, 'include'), tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]


def _call_sites():
    files = ([os.path.join(ROOT, 'bench.py')] + glob.glob(os.path.join(ROOT, 'tools', '*.py')) +
             glob.glob(os.path.join(ROOT, 'tests', '*.py')) +
             glob.glob(os.path.join(os.path.dirname(_lib.__file__), '**', '*.py'), recursive=True))
    for path in sorted(files):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in _lib.SYMBOLS:
                yield f'{os.path.relpath(path, ROOT)}:{node.lineno}', node.func.attr, node


def test_every_call_site_passes_the_declared_arguments():
    """ctypes accepts surplus arguments of a cdecl call and the library would read a missing one from a stale register:
    neither fails in Python, so the count is checked here."""
    seen, starred, wrong = {}, [], []
    for where, name, call in _call_sites():
        if any(isinstance(a, ast.Starred) for a in call.args):
            starred.append(where)
            continue
        seen[where] = name
        want = len(_lib.SYMBOLS[name][1])
        if call.keywords or len(call.args) != want:
            wrong.append(f'{where}: {name} takes {want} positional arguments, the call passes {len(call.args)}'
                         f' and {len(call.keywords)} keywords')
    print(f'{len(seen)} call sites of {len(set(seen.values()))} symbols; not counted (* arguments): {starred}')
    assert not wrong, '\n'.join(wrong)
    assert len(seen) >= 200 and len(set(seen.values())) >= 120, (len(seen), len(set(seen.values())))
