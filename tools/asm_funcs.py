#!/usr/bin/env python3
"""Compare the device functions of two sets of gfx950 assembly files.

The files come from the Makefile's HIPFLAGS plus --cuda-device-only -S:

    hipcc -O3 -fPIC --offload-arch=gfx950 -std=c++17 -Wno-unused-result \\
          --cuda-device-only -S hip/engine.hip -o engine.s

Each file is split by function symbol (.type NAME,@function): the body from
the symbol's label to its .Lfunc_end and, for a kernel, its .amdhsa_kernel
descriptor block.  The <n> of .LBB<n>_ labels, and of the BB<n>_ in the loop
comments, is removed (it counts the functions of a file), and runs of blanks
become one (the comment column moves with that number's width).  A function's
text must then be the same on both sides.

    asm_funcs.py --a parent/engine.s --b engine.s exports.s [--same OLD=NEW ...]

prints identical / different / only-in-one by demangled name and exits non-zero
on any difference, or when a function is defined in two files of one side.
--same OLD=NEW treats the symbol OLD of side A as NEW of side B (a variable
that changed linkage, say).  Text is compared; no instruction is looked for.
"""
import argparse
import re
import subprocess
import sys

TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
LABEL = re.compile(r"^([^\s:;]+):")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
KERNEL_END = re.compile(r"^\s*\.end_amdhsa_kernel")
LBB = re.compile(r"(?:(?<=\.L)|(?<![\w.]))BB\d+_")


def functions(path):
    """{symbol: text} of one assembly file; a kernel's text ends with its descriptor"""
    names, body, desc = [], {}, {}
    cur, kern = None, None
    for line in open(path):
        line = re.sub(r"[ \t]+", " ", LBB.sub("BB_", line.rstrip()))
        m = TYPE.match(line)
        if m:
            names.append(m.group(1))
        m = LABEL.match(line)
        if cur is None and m and m.group(1) in names and m.group(1) not in body:
            cur = m.group(1)
            body[cur] = []
        if cur is not None:
            if FUNC_END.match(line):
                cur = None
            else:
                body[cur].append(line)
        m = KERNEL.match(line)
        if m:
            kern = m.group(1)
            desc[kern] = []
        if kern is not None:
            desc[kern].append(line)
            if KERNEL_END.match(line):
                kern = None
    missing = [n for n in names if n not in body]
    if missing:
        sys.exit(f"{path}: no body found for {missing[:3]}")
    return {n: "\n".join(body[n] + desc.get(n, [])) for n in body}, set(desc)


def side(paths):
    funcs, kernels, clash = {}, set(), []
    for p in paths:
        f, k = functions(p)
        clash += [n for n in f if n in funcs]
        funcs.update(f)
        kernels |= k
    return funcs, kernels, clash


def demangle(names):
    names = list(names)
    if not names:
        return {}
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, out.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True, metavar="FILE", help="assembly files of side A")
    ap.add_argument("--b", nargs="+", required=True, metavar="FILE", help="assembly files of side B")
    ap.add_argument("--same", action="append", default=[], metavar="OLD=NEW",
                    help="symbol OLD of side A is symbol NEW of side B")
    ap.add_argument("-v", "--verbose", action="store_true", help="list the identical functions too")
    args = ap.parse_args()

    fa, ka, clash_a = side(args.a)
    fb, kb, clash_b = side(args.b)
    for pair in args.same:
        old, new = pair.split("=", 1)
        word = re.compile(r"(?<![\w$.])" + re.escape(old) + r"(?![\w$.])")
        fa = {n: word.sub(new, t) for n, t in fa.items()}

    both = sorted(set(fa) & set(fb))
    same = [n for n in both if fa[n] == fb[n]]
    diff = [n for n in both if fa[n] != fb[n]]
    only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    nice = demangle(set(fa) | set(fb))

    print(f"function symbols   A {len(fa)} ({len(ka)} kernels)   B {len(fb)} ({len(kb)} kernels)")
    for p in args.b:
        print(f"  of B in {p}: {len(functions(p)[0])}")
    print(f"identical          {len(same)}")
    print(f"different          {len(diff)}")
    print(f"only in A          {len(only_a)}")
    print(f"only in B          {len(only_b)}")
    print(f"defined twice      A {len(clash_a)}   B {len(clash_b)}")
    if args.verbose:
        for n in same:
            print(f"  identical  {nice[n]}")
    for tag, names in (("different", diff), ("only in A", only_a), ("only in B", only_b),
                       ("twice in A", clash_a), ("twice in B", clash_b)):
        for n in names:
            print(f"  {tag}  {nice[n]}")
    return 1 if diff or only_a or only_b or clash_a or clash_b else 0


if __name__ == "__main__":
    sys.exit(main())
