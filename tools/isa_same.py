#!/usr/bin/env python3
"""Are the recurrent kernels' instruction streams what they were at another commit?  A review aid for changes to
lstm-rnn_amd/csrc/cn_lstm_device.h and the three files that include it (a refactor there should change no kernel): compiles
cn_lstm.hip, cn_lstm_s2.hip and cn_lstm_cluster.hip to gfx950 assembly with the Makefile's flags, once from the working tree
and once from REV, and compares per kernel symbol the instruction sequence (comments, debug directives and label numbers
stripped) and the register / scratch / LDS figures of the kernel metadata.  No GPU needed; not a test.

usage: python tools/isa_same.py [REV=HEAD] [FILE[:-DDEFINE] ...]      e.g.  tools/isa_same.py HEAD~1 cn_lstm:-DCN_STAMP
default configurations: the three files plain, and with the defines of tools/stamps*.py
"""
import concurrent.futures as cf, os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "lstm-rnn_amd/csrc"
CONFIGS = ["cn_lstm", "cn_lstm_s2", "cn_lstm_cluster", "cn_lstm:-DCN_STAMP", "cn_lstm_s2:-DCN_S2_STAMP",
           "cn_lstm_cluster:-DCN_CL_STAMP", "cn_lstm_cluster:-DCN_S2C_STAMP"]
FIGURES = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".vgpr_spill_count"]


def emit(src_root, config, out):
    name, _, define = config.partition(":")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out]
                   + ([define] if define else []) + [os.path.join(src_root, CSRC, name + ".hip")], check=True, capture_output=True)
    return out


def kernels(path):
    """{symbol: (instruction lines, {figure: value})} of one assembly file"""
    text = open(path).read()
    figures = {}
    for entry in re.split(r"\n  - (?=\.agpr_count)", text.split("amdhsa.kernels:")[1]):
        sym = re.search(r"\n    \.symbol:\s+(\S+)\.kd", entry)
        if sym:
            figures[sym.group(1)] = {f: int(re.search(r"(?:^|\s)" + re.escape(f) + r":\s+(\d+)", entry).group(1)) for f in FIGURES}
    streams = {}
    for sym, body in re.findall(r"\n(\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", text, re.S):
        if sym not in figures:
            continue
        lines = []
        for line in body.split("\n"):
            line = re.sub(r"\.L(BB|tmp)\d+", r".L\1", line.split(";")[0]).strip()
            if line and not re.match(r"\.(loc|file|cfi_|ident|p2align|Lfunc_begin)", line):
                lines.append(line)
        streams[sym] = lines
    return {s: (streams[s], figures[s]) for s in figures}


def compare(old, new, label):
    a, b = kernels(old), kernels(new)
    differs = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            print("%-28s %s: only in %s" % (label, sym, "REV" if sym in a else "the working tree")); differs += 1
            continue
        same = a[sym] == b[sym]
        differs += not same
        f = b[sym][1]
        print("%-28s %6d instr  v%-3d a%-3d s%-3d scratch %-4d lds %-6d spill %d  %s  %s" % (
            label, len(b[sym][0]), *[f[k] for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size",
                                                   ".group_segment_fixed_size", ".vgpr_spill_count")], "same   " if same else "DIFFERS", sym))
    return len(b), differs


def main(argv):
    rev = argv[0] if argv else "HEAD"
    configs = argv[1:] or CONFIGS
    with tempfile.TemporaryDirectory() as tmp:
        old_root = os.path.join(tmp, "rev")
        os.makedirs(old_root)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old_root], input=tar, check=True)
        with cf.ThreadPoolExecutor(max_workers=min(os.cpu_count() or 2, 8)) as pool:
            jobs = {c: (pool.submit(emit, old_root, c, os.path.join(tmp, "old%d.s" % i)), pool.submit(emit, ROOT, c, os.path.join(tmp, "new%d.s" % i)))
                    for i, c in enumerate(configs)}
            total = bad = 0
            for c, (o, n) in jobs.items():
                k, d = compare(o.result(), n.result(), c)
                total += k; bad += d
    print("%d kernel symbols, %d differ from %s" % (total, bad, rev))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
