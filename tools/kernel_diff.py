#!/usr/bin/env python
"""Compare the gfx950 device code of two builds of the library, kernel by kernel: the "same code" proof of a refactor.

Both libraries are unbundled and disassembled the way tools/scan_isa.py does it (host only: llvm-objcopy,
clang-offload-bundler, llvm-objdump --demangle).  A kernel's text is its instruction lines without the address /
encoding comment, with symbol references (<name+0x..>) and local label numbers (.LBB12_3) masked, so that a kernel that
merely moved or was renamed compares equal; the padding behind a kernel's last instruction is not part of it.  --rename
maps names of the FIRST library onto the second's.

    python tools/kernel_diff.py OLD.so NEW.so [--rename 'REGEX=REPLACEMENT' ...] [--resources OLD.json NEW.json]

Prints the kernel count of each side, the kernels present on one side only and the first differing lines of every kernel
whose text differs; with --resources also every entry of the two kernel_resources*.json reports (registers, scratch, LDS)
that differs under the same renames.  Exit status 0: no difference; 1: any."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_isa  # noqa: E402

SHOWN = 6                                   # differing lines printed per kernel
PADDING = ('s_nop 0', 's_code_end', '...')  # what the assembler and objdump put between one kernel's end and the next


def code_objects(so_path, tmp):
    """The gfx950 code objects of every offload bundle of the library's .hip_fatbin (scan_isa.scan's extraction)."""
    fat = os.path.join(tmp, 'fat.bin')
    subprocess.run([os.path.join(scan_isa.LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, so_path,
                    os.path.join(tmp, 'discarded_copy.so')], check=True)
    blob = open(fat, 'rb').read()
    starts = [m.start() for m in re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', blob)] + [len(blob)]
    for i in range(len(starts) - 1):
        part, co = os.path.join(tmp, 'b%d.bin' % i), os.path.join(tmp, 'b%d.co' % i)
        with open(part, 'wb') as f:
            f.write(blob[starts[i]:starts[i + 1]])
        subprocess.run([os.path.join(scan_isa.LLVM, 'clang-offload-bundler'), '--type=o',
                        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + part, '--output=' + co, '--unbundle'],
                       check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        yield co


def kernels(so_path):
    """{demangled name without argument list: [masked instruction lines]} of a library."""
    tmp = tempfile.mkdtemp()
    out = {}
    try:
        for co in code_objects(so_path, tmp):
            dis = subprocess.run([os.path.join(scan_isa.LLVM, 'llvm-objdump'), '-d', '--demangle', co], check=True,
                                 stdout=subprocess.PIPE, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r'^[0-9a-f]+ <(.*)>:', line)
                if m:
                    name = m.group(1).split('(')[0].replace('void ', '')
                    while name in out:                      # overloads that differ in their arguments only
                        name += "'"
                    cur = out[name] = []
                elif cur is not None and line.startswith(('\t', ' ')) and line.strip():
                    cur.append(mask(line))
        for text in out.values():                           # the fill up to the next symbol's alignment is no code
            while text and text[-1] in PADDING:
                text.pop()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def mask(line):
    t = line.split('//')[0].strip()
    t = re.sub(r'<[^<>]*(?:<[^<>]*>[^<>]*)*>', '<sym>', t)
    return re.sub(r'\.L[A-Za-z_]*\d+(?:_\d+)?', '.L', t)


def renamer(rules):
    pairs = []
    for r in rules:
        pat, _, rep = r.partition('=')
        pairs.append((re.compile(pat), rep))

    def rename(name):
        for pat, rep in pairs:
            new, n = pat.subn(rep, name)
            if n:
                return new
        return name
    return rename


def diff_sets(kind, a, b):
    """Names on one side only; returns their number."""
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    for side, names in (('first', only_a), ('second', only_b)):
        for n in names:
            print('%s only in the %s: %s' % (kind, side, n))
    return len(only_a) + len(only_b)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--rename', action='append', default=[], metavar='REGEX=REPLACEMENT',
                    help='applied (re.sub, first rule that matches) to the kernel names of the first library')
    ap.add_argument('--resources', nargs=2, metavar=('OLD.json', 'NEW.json'))
    args = ap.parse_args()
    rename = renamer(args.rename)

    a = {rename(k): v for k, v in kernels(args.old).items()}
    b = kernels(args.new)
    print('kernels: %d in %s, %d in %s' % (len(a), args.old, len(b), args.new))
    bad = diff_sets('kernel', a, b)
    differing = 0
    for name in sorted(set(a) & set(b)):
        if a[name] == b[name]:
            continue
        differing += 1
        print('kernel differs: %s (%d / %d lines)' % (name, len(a[name]), len(b[name])))
        shown = 0
        for i in range(max(len(a[name]), len(b[name]))):
            la = a[name][i] if i < len(a[name]) else '<end>'
            lb = b[name][i] if i < len(b[name]) else '<end>'
            if la != lb:
                print('  line %d:\n    - %s\n    + %s' % (i + 1, la, lb))
                shown += 1
                if shown == SHOWN:
                    break
    print('%d of %d common kernels differ' % (differing, len(set(a) & set(b))))
    bad += differing

    if args.resources:
        ra = {rename(k): v for k, v in json.load(open(args.resources[0])).items()}
        rb = json.load(open(args.resources[1]))
        bad += diff_sets('resource entry', ra, rb)
        entries = 0
        for name in sorted(set(ra) & set(rb)):
            if ra[name] != rb[name]:
                entries += 1
                print('resources differ: %s\n    - %s\n    + %s' % (name, ra[name], rb[name]))
        print('resource entries: %d / %d, %d differ' % (len(ra), len(rb), entries))
        bad += entries
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
