#!/usr/bin/env python3
"""Compares the gfx950 device code of two builds, kernel by kernel.

    tools/kernel_diff.py OLD.o... -- NEW.o...

Each hipcc object's gfx950 code object is extracted (llvm-objdump --offloading)
and its kernels listed (llvm-readelf -sW: FUNC symbols and their .kd
descriptors).  For every kernel of either side the symbol size, the 64
descriptor bytes and the disassembly (addresses and encodings stripped) are
compared; one line per kernel: same, differs, missing or duplicated.  Exit
status 0 only when every kernel is `same`.

Two things move with a kernel's address and are compared by what they point at,
not by their bytes (the output's header says so): the literal of an
s_getpc_b64 / s_add_u32 / s_addc_u32 address (shown as <symbol + offset>: a data symbol by its
unqualified name, or the kernel itself for a long branch), and the descriptor's kernel_code_entry_byte_offset (bytes 16..23, compared as
the kernel it lands on).  Nothing else is masked.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True,
                          text=True, cwd=cwd).stdout


def symbols(co, demangle):
    """[(value, size, type, name)] of the code object's .symtab (readelf lists .dynsym first)."""
    out, on = [], False
    for line in run('llvm-readelf', '-sW', *(['-C'] if demangle else []), co).splitlines():
        if line.startswith('Symbol table'):
            on = "'.symtab'" in line
        f = line.split(None, 7)
        if on and len(f) == 8 and f[0].rstrip(':').isdigit() and f[3] in ('FUNC', 'OBJECT') and f[6] != 'UND':
            out.append((int(f[1], 16), int(f[2]), f[3], f[7]))
    return out


def section(co, name):
    """(address, file offset) of a section."""
    for line in run('llvm-readelf', '-SW', co).splitlines():
        m = re.match(r'\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)', line)
        if m and m.group(1) == name:
            return int(m.group(2), 16), int(m.group(3), 16)
    raise SystemExit(f'{co}: no {name} section')


INS = re.compile(r'^\s+(\S.*?)\s+// ([0-9A-F]+): ')


def disassembly(co, sym, end, data):
    """The kernel's instructions as text up to its end (the padding behind it
    is the next symbol's alignment); pc-relative literals resolved to symbols."""
    def where(addr):
        for v, s, name in data:
            if v <= addr < v + max(s, 1):
                return f'<{name}+{addr - v}>'
        return f'<unknown {addr:#x}>'
    out, pc, reg = [], None, None
    for line in run('llvm-objdump', '-d', f'--disassemble-symbols={sym}', co).splitlines():
        m = INS.match(line)
        if not m:
            continue
        ins, addr = m.group(1), int(m.group(2), 16)
        if addr >= end:
            break
        g = re.match(r's_getpc_b64 s\[(\d+):(\d+)\]$', ins)
        a = re.match(r's_add_u32 s(\d+), s(\d+), (0x[0-9a-f]+|\d+)$', ins)
        c = re.match(r's_addc_u32 s(\d+), s(\d+), (0x[0-9a-f]+|-?\d+)$', ins)
        if g:
            pc, reg = addr + 4, (g.group(1), g.group(2))
        elif a and reg and a.group(1) == a.group(2) == reg[0]:
            lit = int(a.group(3), 0)
            ins = f's_add_u32 s{reg[0]}, s{reg[0]}, {where(pc + (lit - (1 << 32) if lit >> 31 else lit))}'
        elif c and reg and c.group(1) == c.group(2) == reg[1]:
            ins, reg = f's_addc_u32 s{reg[1]}, s{reg[1]}, <high half>', None
        else:
            reg = None
        out.append(ins)
    return out


def kernels(obj, tmp, tag):
    """{kernel: [(size, descriptor, entry, disassembly)]} of one hipcc object."""
    d = os.path.join(tmp, tag)
    os.makedirs(d)
    shutil.copy(obj, os.path.join(d, 'a.o'))
    run('llvm-objdump', '--offloading', 'a.o', cwd=d)
    cos = [os.path.join(d, f) for f in os.listdir(d) if 'gfx950' in f]
    if len(cos) != 1:
        raise SystemExit(f'{obj}: {len(cos)} gfx950 code objects')
    co = cos[0]
    syms = symbols(co, False)
    # (data symbols by their unqualified name: each unit has its own namespace for its copies)
    data = [(v, s, n.split('::')[-1]) for v, s, t, n in symbols(co, True) if t == 'OBJECT' and '.kd' not in n]
    data += [(v, s, n) for v, s, t, n in syms if t == 'FUNC']
    ro_addr, ro_off = section(co, '.rodata')
    blob = open(co, 'rb').read()
    funcs = {n: (v, s) for v, s, t, n in syms if t == 'FUNC'}
    res = {}
    for v, s, t, n in syms:
        if t != 'OBJECT' or not n.endswith('.kd'):
            continue
        k = n[:-3]
        if k not in funcs or s != 64:
            raise SystemExit(f'{obj}: descriptor {n} without its kernel')
        kd = blob[ro_off + v - ro_addr:][:64]
        entry = v + int.from_bytes(kd[16:24], 'little', signed=True) - funcs[k][0]
        res.setdefault(k, []).append((funcs[k][1], kd[:16] + kd[24:], entry, disassembly(co, k, sum(funcs[k]), data)))
    return res


def main():
    if '--' not in sys.argv:
        raise SystemExit(__doc__)
    i = sys.argv.index('--')
    sides = sys.argv[1:i], sys.argv[i + 1:]
    with tempfile.TemporaryDirectory() as tmp:
        found = []
        for s, objs in enumerate(sides):
            ks = {}
            for j, o in enumerate(objs):
                for k, v in kernels(o, tmp, f'{s}_{j}').items():
                    ks.setdefault(k, []).extend((os.path.basename(o), x) for x in v)
            found.append(ks)
    old, new = found
    print('# old:', ' '.join(sides[0]))
    print('# new:', ' '.join(sides[1]))
    print('# compared per kernel: symbol size, descriptor bytes, disassembly without addresses and encodings')
    print('# masked: the literal of s_getpc_b64 address pairs (compared as symbol + offset) and the')
    print('#         descriptor\'s kernel_code_entry_byte_offset (compared as an offset into its kernel)')
    count = {}
    for k in sorted(set(old) | set(new)):
        what, unit = 'same', ','.join(o for o, _ in new.get(k, []))
        if len(old.get(k, [])) > 1 or len(new.get(k, [])) > 1:
            what = 'duplicated'
        elif k not in old or k not in new:
            what = 'missing'
            unit = 'only in ' + ('old' if k in old else 'new')
        elif old[k][0][1] != new[k][0][1]:
            (sa, da, ea, ta), (sb, db, eb, tb) = old[k][0][1], new[k][0][1]
            why = [w for w, x, y in (('size', sa, sb), ('descriptor', da, db), ('entry', ea, eb),
                                     ('code', ta, tb)) if x != y]
            what = 'differs (' + ', '.join(why) + ')'
            if ta != tb:
                n = next((j for j, (x, y) in enumerate(zip(ta, tb)) if x != y), min(len(ta), len(tb)))
                what += f' at instruction {n}: {ta[n:n + 1]} -> {tb[n:n + 1]}'
        count[what.split()[0]] = count.get(what.split()[0], 0) + 1
        print(f'{what:10s} {unit:18s} {k}')
    print('#', len(old), 'old kernels,', len(new), 'new kernels:',
          ', '.join(f'{n} {w}' for w, n in sorted(count.items())))
    return 0 if set(count) <= {'same'} and count else 1


if __name__ == '__main__':
    sys.exit(main())
