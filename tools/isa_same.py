#!/usr/bin/env python3
"""Compares the gfx950 code of two builds, symbol by symbol:  tools/isa_same.py OLD_DIR NEW_DIR

OLD_DIR / NEW_DIR hold the kernels_*.o of a build (glaze_amd/csrc/build of two checkouts, each built with `make`).  For every kernel and
device function in OLD's objects the same symbol is looked up in NEW -- in the object of the same name first, then in whichever object
holds it (code that moved to another file) -- and the two disassemblies are compared; the line says `same`, `differs` or `missing`,
followed, for a kernel, by the code object's figures in both builds (as tools/isa_meta.sh prints them): VGPRs, VGPR spills, scratch
bytes, LDS bytes.  What does not count as a difference is what moves with the position of the code and not with the code: the address /
encoding comments, the literals of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 (the pc-relative distance to a function that is
called, not inlined), and the padding behind a symbol's last s_endpgm.  Exit status 1 when a symbol differs or is missing.  A symbol
that only NEW has is listed as `new` with its figures and does not count.
With --pair 'OLD NAME=NEW NAME' (demangled kernel names without their arguments, any number of times) nothing else is compared: each
OLD kernel is held against the NEW kernel of another name that replaces it -- `same` (the same instructions in the same order),
`operands` (the same mnemonics in the same order; some operand differs, as a kernel argument's offset does when the argument list
changed), `reordered` (the same number of instructions and the same multiset of mnemonics), or `differs` -- with both instruction counts and
the figures, SGPRs included.  Exit status 1 when a pair differs, a figure differs or a name is not found.
(The .o is a fat binary: llvm-objdump --offloading extracts the device ELF first, as in tools/isa_dump.sh.)
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib/llvm/bin')
FIGURES = [('vgpr', '.vgpr_count'), ('vgpr_spill', '.vgpr_spill_count'), ('scratch', '.private_segment_fixed_size'), ('lds', '.group_segment_fixed_size')]


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def normalise(lines):
    """The instructions of one symbol without what depends on where the code sits."""
    out, pcrel = [], 0
    for line in lines:
        ins = line.split('//')[0].strip()
        if not ins or ins == '...':
            continue
        if ins.startswith('s_getpc_b64'):
            pcrel = 2
        elif pcrel and re.match(r's_addc?_u32 ', ins):
            ins = ins.rsplit(',', 1)[0] + ', <pc-relative>'
            pcrel -= 1
        out.append(ins)
    last = max((i for i, ins in enumerate(out) if ins.startswith('s_endpgm')), default=None)
    if last is not None and all(ins.startswith('s_nop') for ins in out[last + 1:]):
        del out[last + 1:]
    return out


def load(directory):
    """{object name: {symbol: (instructions, figures or None)}} of the kernels_*.o in `directory` (or in its build/)."""
    objects = sorted(glob.glob(os.path.join(directory, 'kernels_*.o'))) or sorted(glob.glob(os.path.join(directory, 'build', 'kernels_*.o')))
    if not objects:
        sys.exit('no kernels_*.o in %s' % directory)
    build = {}
    for obj in objects:
        tmp = tempfile.mkdtemp()
        try:
            shutil.copy(obj, os.path.join(tmp, 'in.o'))
            run(os.path.join(LLVM, 'llvm-objdump'), '--offloading', 'in.o', cwd=tmp)
            elf = glob.glob(os.path.join(tmp, 'in.o.*gfx950*'))[0]
            figures, name = {}, None
            for line in run(os.path.join(LLVM, 'llvm-readelf'), '--notes', elf).splitlines():
                m = re.match(r'\s+(?:- )?(\.[a-z_]+):\s+(\S+)\s*$', line)
                if not m:
                    continue
                if line.startswith('  - '):   # a new entry of amdhsa.kernels
                    name, pending = None, {}
                if m.group(1) == '.name' and not line.startswith('      '):
                    name = m.group(2)
                    figures[name] = pending
                elif not line.startswith('      '):   # (six spaces: a field of one of the kernel's arguments)
                    (figures[name] if name else pending)[m.group(1)] = m.group(2)
            symbols, current = {}, None
            for line in run(os.path.join(LLVM, 'llvm-objdump'), '-d', '--mcpu=gfx950', elf).splitlines():
                m = re.match(r'[0-9a-f]+ <(.+)>:$', line)
                if m:
                    current = symbols.setdefault(m.group(1), [])
                elif current is not None and line.startswith('\t'):
                    current.append(line)
            build[os.path.basename(obj)] = {s: (normalise(l), figures.get(s)) for s, l in symbols.items()}
        finally:
            shutil.rmtree(tmp)
    return build


def pairs(old, new, wanted, filt):
    """The --pair mode: kernels of OLD against the kernels of NEW that replace them under another name."""
    def by_name(build):
        syms = [(s, v) for o in build.values() for s, v in o.items() if v[1] is not None]
        return {re.sub(r'\(.*', '', n).replace('void ', ''): v for (s, v), n in zip(syms, run(filt, *[s for s, _ in syms]).splitlines())}
    old, new, bad = by_name(old), by_name(new), 0
    figures = FIGURES + [('sgpr', '.sgpr_count')]
    for pair in wanted:
        a, b = (x.strip() for x in pair.split('='))
        if a not in old or b not in new:
            print('%-10s%s = %s' % ('not found', a, b))
            bad += 1
            continue
        (code, fig), (code2, fig2) = old[a], new[b]
        m, m2 = [i.split()[0] for i in code], [i.split()[0] for i in code2]
        verdict = 'same' if code == code2 else 'operands' if m == m2 else 'reordered' if sorted(m) == sorted(m2) else 'differs'
        differ = any(fig.get(key) != fig2.get(key) for _, key in figures)
        bad += verdict == 'differs' or differ
        print('%-10s%s = %s  instructions %d/%d  %s%s' % (verdict, a, b, len(code), len(code2), '  '.join('%s %s/%s' % (label, fig.get(key, '-'), fig2.get(key, '-')) for label, key in figures),
                                                       '  FIGURES DIFFER' if differ else ''))
    print('%d pairs: %s' % (len(wanted), 'none differs' if not bad else '%d not' % bad))
    return 1 if bad else 0


def main():
    wanted = [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == '--pair']
    if len(sys.argv) != 3 + 2 * len(wanted) or '--pair' in sys.argv[1:3]:
        sys.exit(__doc__)
    old, new = load(sys.argv[1]), load(sys.argv[2])
    if wanted:
        return pairs(old, new, wanted, shutil.which('llvm-cxxfilt', path=LLVM) or shutil.which('c++filt'))
    names = [s for syms in old.values() for s in syms]
    filt = shutil.which('llvm-cxxfilt', path=LLVM) or shutil.which('c++filt')   # readable names where a demangler is at hand
    plain = dict(zip(names, run(filt, *names).splitlines() if filt and names else names))
    bad = 0
    for obj, syms in old.items():
        for sym, (code, fig) in syms.items():
            where = obj if sym in new.get(obj, {}) else next((o for o in new if sym in new[o]), None)
            if where is None:
                verdict, fig2 = 'missing', None
            else:
                code2, fig2 = new[where][sym]
                verdict = 'same' if code == code2 else 'differs'
            bad += verdict != 'same'
            text = '%-8s%s  [%s -> %s]' % (verdict, re.sub(r'\(.*', '', plain[sym]), obj, where or '-')
            if fig is not None:
                text += '  ' + '  '.join('%s %s/%s' % (label, fig.get(key, '-'), (fig2 or {}).get(key, '-')) for label, key in FIGURES)
                if fig2 is not None and any(fig.get(key) != fig2.get(key) for _, key in FIGURES):
                    text += '  FIGURES DIFFER'
                    bad += 1
            print(text)
    for obj, syms in new.items():   # what NEW has and OLD has not, with a kernel's figures: reported, not counted
        fresh = [s for s in syms if not any(s in o for o in old.values())]
        for sym, name in zip(fresh, run(filt, *fresh).splitlines() if filt and fresh else fresh):
            fig = syms[sym][1]
            print('%-8s%s  [- -> %s]' % ('new', re.sub(r'\(.*', '', name), obj) + ('' if fig is None else '  ' + '  '.join('%s -/%s' % (label, fig.get(key, '-')) for label, key in FIGURES)))
    print('%d symbols of %s compared with %s: %s' % (len(names), sys.argv[1], sys.argv[2], 'all same' if not bad else '%d not the same' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
