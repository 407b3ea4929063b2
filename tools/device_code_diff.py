#!/usr/bin/env python3
"""Compare the gfx950 device code that two trees build from the same csrc/*.hip files.

    tools/device_code_diff.py REV_A REV_B [FILE.hip ...]

A tree is a git revision (materialised with `git archive` into a temporary directory) or `.`, the
working tree (its tracked and its new, not ignored files, copied likewise).  Every named file (default: the translation units that include mlp_core.h /
mlp_stream.h / mtl_core.h) is compiled in each tree with the flags that tree's csrc/Makefile gives its library
objects (read from `make -n`), plus --offload-device-only --no-gpu-bundle-output, at most 16
compiles at once.  One line per file: `identical` when the two device ELFs have the same sha256,
otherwise the __global__ kernels whose instruction stream (llvm-objdump -d, addresses and encodings
stripped) or metadata (llvm-readelf --notes) differs, and the kernels added or missing.  A file that
only one of the trees has (a translation unit added or removed between them) is reported as such and
compared with nothing.  The exit status is non-zero unless every file both trees have is identical.
Host only: needs hipcc, no GPU.
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

DEFAULT_FILES = ["mlp.hip", "din_fused.hip", "deepfm_fused.hip", "bst_small.hip", "dien_forward.hip",
                 "linear_tiled.hip", "afm.hip", "mmoe.hip", "ple.hip", "esmm.hip"]
DEVICE_ONLY = ["--offload-device-only", "--no-gpu-bundle-output"]
# per-kernel metadata named in a report (any other difference in the kernel's note is "other")
META_KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size",
             ".private_segment_fixed_size", ".kernarg_segment_size"]
MAX_JOBS = 16
ELF_DIR = "device_elf"


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, **kw).stdout


def materialise(rev, repo, tmp, side):
    """A copy of tree `rev` under tmp: an archive of the revision, or for `.` the working tree's
    tracked and untracked-but-not-ignored files.  Both trees are compiled from copies with the same
    relative command line: hipcc derives the name of one symbol per translation unit (__hip_cuid_*)
    from the command line as given, so an output path that differs would alone change the hash."""
    root = os.path.join(tmp, f"tree_{side}")
    os.makedirs(root)
    if rev == ".":
        listed = run(["git", "-C", repo, "ls-files", "-z", "-c", "-o", "--exclude-standard"]).split("\0")
        for f in listed:
            src = os.path.join(repo, f)
            if f and os.path.isfile(src) and not os.path.islink(src):
                os.makedirs(os.path.dirname(os.path.join(root, f)), exist_ok=True)
                shutil.copyfile(src, os.path.join(root, f))
        return root
    archive = subprocess.Popen(["git", "-C", repo, "archive", rev], stdout=subprocess.PIPE)
    subprocess.run(["tar", "-x", "-C", root], stdin=archive.stdout, check=True)
    if archive.wait() != 0:
        sys.exit(f"git archive {rev} failed")
    return root


def find_csrc(root):
    for d, dirs, files in os.walk(root):
        dirs[:] = [x for x in dirs if x not in (".git", "build")]
        if os.path.basename(d) == "csrc" and "Makefile" in files:
            return d
    sys.exit(f"no csrc/Makefile under {root}")


def compile_command(csrc, name, out):
    """The Makefile's compile line of csrc/<name> as an argv that writes the device ELF to `out`."""
    obj = "build/" + name[: -len(".hip")] + ".o"
    text = run(["make", "-n", "-B", "BUILD=build", obj], cwd=csrc)
    for line in text.splitlines():
        argv = shlex.split(line)
        if "-c" in argv and name in argv and "-o" in argv:
            i = argv.index("-o")
            return argv[:i] + argv[i + 2:] + DEVICE_ONLY + ["-o", out]
    sys.exit(f"no compile line for {name} in `make -n` of {csrc}")


def kernels_of(elf, llvm_bin):
    """{kernel: (instruction text, metadata block)} of a device ELF."""
    notes = run([os.path.join(llvm_bin, "llvm-readelf"), "--notes", elf])
    meta, block, in_kernels = {}, None, False

    def close(b):
        if b:
            m = re.search(r"^\s+\.name:\s+(\S+)", "\n".join(b), re.M)
            if m:
                meta[m.group(1)] = "\n".join(b)

    for line in notes.splitlines():
        if re.match(r"\s*amdhsa\.kernels:", line):
            in_kernels = True
        elif in_kernels and re.match(r"\s{0,2}amdhsa\.", line):
            in_kernels = False
            close(block)
            block = None
        elif in_kernels and re.match(r"  - ", line):
            close(block)
            block = [line]
        elif in_kernels and block is not None:
            block.append(line)
    close(block)

    code, cur = {}, None
    for line in run([os.path.join(llvm_bin, "llvm-objdump"), "-d", elf]).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = code.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(line.split("//")[0].strip())
    return {k: ("\n".join(code.get(k, [])), v) for k, v in meta.items()}


def meta_fields(block):
    return {k: (re.search(r"^\s+(?:- )?" + re.escape(k) + r":\s+(\S+)", block, re.M) or [None, None])[1]
            for k in META_KEYS}


def compare(name, elf_a, elf_b, llvm_bin):
    sha = [hashlib.sha256(open(e, "rb").read()).hexdigest() for e in (elf_a, elf_b)]
    if sha[0] == sha[1]:
        return True, f"{name}: identical  sha256 {sha[0]}"
    ka, kb = kernels_of(elf_a, llvm_bin), kernels_of(elf_b, llvm_bin)
    parts = []
    code = sorted(k for k in ka.keys() & kb.keys() if ka[k][0] != kb[k][0])
    metas = []
    for k in sorted(ka.keys() & kb.keys()):
        if ka[k][1] != kb[k][1]:
            fa, fb = meta_fields(ka[k][1]), meta_fields(kb[k][1])
            changed = [f"{f} {fa[f]} -> {fb[f]}" for f in META_KEYS if fa[f] != fb[f]] or ["other"]
            metas.append(f"{k} ({', '.join(changed)})")
    for label, items in (("instructions differ", code), ("metadata differs", metas),
                         ("added", sorted(kb.keys() - ka.keys())), ("missing", sorted(ka.keys() - kb.keys()))):
        parts.append(f"{label}: {len(items)}" + (" [" + "; ".join(items) + "]" if items else ""))
    return False, f"{name}: DIFFERENT  sha256 {sha[0][:16]} / {sha[1][:16]}  of {len(ka)} kernels " + ", ".join(parts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev_a", help="git revision, or . for the working tree")
    ap.add_argument("rev_b", help="git revision, or . for the working tree")
    ap.add_argument("files", nargs="*", default=DEFAULT_FILES, help="csrc/*.hip files (default: %(default)s)")
    ap.add_argument("-j", "--jobs", type=int, default=MAX_JOBS, help="compiles at once (at most %d)" % MAX_JOBS)
    args = ap.parse_args()
    repo = run(["git", "-C", os.path.dirname(os.path.abspath(__file__)), "rev-parse", "--show-toplevel"]).strip()
    names = [os.path.basename(f) for f in args.files]

    with tempfile.TemporaryDirectory(prefix="device_code_diff_") as tmp:
        jobs = []  # (side, name, csrc, argv, elf)
        llvm_bin = None
        for side, rev in enumerate((args.rev_a, args.rev_b)):
            csrc = find_csrc(materialise(rev, repo, tmp, side))
            os.makedirs(os.path.join(csrc, ELF_DIR))
            for name in names:
                if not os.path.isfile(os.path.join(csrc, name)):
                    continue
                elf = os.path.join(ELF_DIR, name + ".elf")  # relative to csrc, the same in both trees
                argv = compile_command(csrc, name, elf)
                llvm_bin = llvm_bin or os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(argv[0]))), "llvm", "bin")
                jobs.append((side, name, csrc, argv, os.path.join(csrc, elf)))
        if not os.path.exists(os.path.join(llvm_bin, "llvm-objdump")):
            llvm_bin = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")

        def build(job):
            r = subprocess.run(job[3], cwd=job[2], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            return job, r

        with concurrent.futures.ThreadPoolExecutor(max(1, min(args.jobs, MAX_JOBS))) as pool:
            for job, r in pool.map(build, jobs):
                if r.returncode != 0:
                    sys.exit(f"compile of {job[1]} in tree {'AB'[job[0]]} failed:\n{r.stdout}")

        all_same = True
        elf = {(side, name): path for side, name, _, _, path in jobs}
        for name in names:
            if (0, name) not in elf or (1, name) not in elf:
                have = [t for i, t in enumerate("AB") if (i, name) in elf]
                print(f"{name}: only in tree {have[0]}" if have else f"{name}: in neither tree", flush=True)
                continue
            same, line = compare(name, elf[0, name], elf[1, name], llvm_bin)
            all_same &= same
            print(line, flush=True)
    return 0 if all_same else 1


if __name__ == "__main__":
    sys.exit(main())
