"""Strict reader of the C ABI header: structs, prototypes and integer constants as ctypes, with no second copy.

The header is regular C: comments, an include guard, the extern "C" bracket, `#define NAME <integer>`, anonymous enums,
`typedef struct { ... } name_t;` and prototypes.  Everything recognised is cut out of the text; whatever is left, and
any type name that is not listed here, raises HeaderError naming it, so a construct this reader does not understand
cannot be bound wrongly."""
from __future__ import annotations

import ctypes as C
import re
from collections import namedtuple

SCALARS = {'void': None, 'char': C.c_char, 'int': C.c_int, 'int16_t': C.c_int16, 'int32_t': C.c_int32,
           'int64_t': C.c_int64, 'float': C.c_float, 'double': C.c_double}
BOILERPLATE = (r'#ifndef[ \t]+(\w+)\s*#define[ \t]+\1[ \t]*\n', r'#include[ \t]*<stdint\.h>',
               r'#ifdef[ \t]+__cplusplus\s*(extern[ \t]+"C"[ \t]*\{|\})\s*#endif', r'#endif')

# one declarator with its declaration's type: `const float *w_l` -> (True, 'float', 1, 'w_l', None); count = array length
Decl = namedtuple('Decl', 'const base depth name count')


class HeaderError(ValueError):
    pass


class Header:
    """structs: name -> ctypes.Structure; fields: name -> [Decl]; functions: name -> (return Decl, [parameter Decl]);
    constants: name -> int; all in the header's order."""

    def __init__(self, text: str):
        self.structs, self.fields, self.functions, self.constants = {}, {}, {}, {}
        text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)         # comments first: they hold ';', '(' and names
        for pattern, handler in ((r'^[ \t]*#define[ \t]+(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$', self._define),
                                 *((p, None) for p in BOILERPLATE),
                                 (r'\benum\s*\{([^{}]*)\}\s*;', self._enum),
                                 (r'\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;', self._struct),
                                 (r'((?:\bconst\s+)?\b\w+[\s*]+)(\w+)\s*\(([^()]*)\)\s*;', self._function)):
            text = re.sub(pattern, lambda m, h=handler: (h and h(m)) or ' ', text, flags=re.M)
        if text.strip():
            raise HeaderError(f'unparsed header text: {text.strip()[:200]!r}')

    def _define(self, m):
        self.constants[m[1]] = int(m[2], 0)

    def _enum(self, m):
        value = -1
        for item in filter(None, (s.strip() for s in m[1].split(','))):
            e = re.fullmatch(r'(\w+)(?:\s*=\s*(-?\w+))?', item)
            if not e:
                raise HeaderError(f'unparsed enumerator: {item!r}')
            value = int(e[2], 0) if e[2] else value + 1
            self.constants[e[1]] = value

    def _decls(self, text):
        """`const float *a, *b` or `mcgen_seg_t seg[2]` -> one Decl per declarator"""
        m = re.fullmatch(r'\s*(const\s+)?(\w+)\b(.*)', text, flags=re.S)
        if not m or (m[2] not in SCALARS and m[2] not in self.structs):
            raise HeaderError(f'unknown type in {text.strip()!r}')
        for d in m[3].split(','):
            dm = re.fullmatch(r'\s*(\**)\s*(\w*)\s*(?:\[(\d+)\])?\s*', d)
            if not dm:
                raise HeaderError(f'unparsed declarator {d.strip()!r} in {text.strip()!r}')
            yield Decl(bool(m[1]), m[2], len(dm[1]), dm[2], int(dm[3]) if dm[3] else None)

    def ctype(self, d: Decl, param: bool = False):
        """Pointers are c_void_p, except a `const char*` and, among parameters, a struct pointer to HOST memory: by the
        header's convention a parameter whose name ends in _dev is a device address, any other struct pointer is host."""
        if d.depth:
            if d.base == 'char':
                return C.c_char_p
            return C.POINTER(self.structs[d.base]) if param and d.base in self.structs and not d.name.endswith('_dev') else C.c_void_p
        t = self.structs.get(d.base) or SCALARS[d.base]
        if t is None and (d.name or d.count):
            raise HeaderError(f'void object {d.name!r}')
        return t * d.count if d.count else t

    def _struct(self, m):
        fields = [d for part in m[1].split(';') if part.strip() for d in self._decls(part)]
        if not all(d.name for d in fields):
            raise HeaderError(f'unnamed field in {m[2]}')
        self.fields[m[2]] = fields
        self.structs[m[2]] = type(m[2], (C.Structure,), {'_fields_': [(d.name, self.ctype(d)) for d in fields]})

    def _function(self, m):
        ret, = self._decls(m[1])
        params = [] if m[3].strip() in ('', 'void') else [d for part in m[3].split(',') for d in self._decls(part)]
        self.functions[m[2]] = (ret, params)

    def symbol(self, name):
        ret, params = self.functions[name]
        return self.ctype(ret), [self.ctype(p, param=True) for p in params]
