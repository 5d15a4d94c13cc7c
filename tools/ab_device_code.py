"""Device-code A/B of two trees of this repository, without a GPU.

    python tools/ab_device_code.py build <tree> <out> [jobs]      every translation unit of <tree> (its own build.py says which) with
        -Rpass-analysis=kernel-resource-usage and -save-temps, each in a directory of its own under <out>: remarks.txt and the assembly;
        then <out>/libi2c_hip.so and <out>/libi2c_hostsim.so, the two libraries tools/ab_bitexact.py compares (ONLY=unit,...: just those
        units, no libraries)
    python tools/ab_device_code.py compare <parent_out> <change_out> [unit,...]
        the kernel symbols of both, the resource figures of the remarks (the fields tools/resusage.py reads, plus spills, LDS and
        occupancy), the kernels whose opcode sequence differs and, of them, those whose largest loop (the time loop of a sweep: the
        method of tools/isa_histogram.py) has another opcode histogram, with the differing counts (parent, change)
"""
import collections, concurrent.futures, importlib.util, os, re, subprocess, sys


def build():
    tree, out = os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])
    jobs = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    spec = importlib.util.spec_from_file_location("b", os.path.join(tree, "input-inference-for-control_amd", "build.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    os.makedirs(out, exist_ok=True)
    def one(tu):
        obj, src, defs = tu
        d = os.path.join(out, obj[:-2]); os.makedirs(d, exist_ok=True)
        cmd = [b.HIPCC] + b.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-save-temps=obj"] + defs + ["-c", os.path.join(b.CSRC, src), "-o", os.path.join(d, obj)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
        open(os.path.join(d, "remarks.txt"), "w").write(r.stdout + r.stderr)
        if r.returncode: raise RuntimeError(" ".join(cmd) + "\n" + r.stderr[-3000:])
        return os.path.join(d, obj)
    only = os.environ.get("ONLY")
    if only:
        with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
            list(pool.map(one, [t for t in b.translation_units() if t[0][:-2] in only.split(",")]))
        sys.exit(0)
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        objs = list(pool.map(one, b.translation_units()))
    subprocess.run([b.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", os.path.join(out, "libi2c_hip.so")], check=True)
    with open(os.path.join(out, "remarks_all.txt"), "w") as f:
        for obj, _, _ in b.translation_units():
            f.write(open(os.path.join(out, obj[:-2], "remarks.txt")).read())
    print("device done", flush=True)
    b.compile_all("g++", b.HOST_SIM_FLAGS, os.path.join(out, "hs_obj"), os.path.join(out, "libi2c_hostsim.so"), ["-shared", "-fPIC"], verbose=False, jobs=jobs)
    print("hostsim done")


def compare():
    pa, ch = sys.argv[2], sys.argv[3]
    tus = sys.argv[4].split(",") if len(sys.argv) > 4 else sorted(d for d in os.listdir(ch) if os.path.isdir(os.path.join(ch, d)) and d != "hs_obj")
    FIELDS = ['AGPRs', 'LDS Size [bytes/block]', 'Occupancy [waves/SIMD]', 'SGPRs Spill', 'ScratchSize [bytes/lane]', 'TotalSGPRs', 'VGPRs', 'VGPRs Spill']
    def res(path):
        out = collections.defaultdict(list)
        for blk in re.split(r'remark: [^\n]*Function Name: ', open(path).read())[1:]:
            name = blk.split('\n')[0].strip()
            out[name].append(tuple(int(m.group(1)) if (m := re.search(re.escape(k) + r': (\d+)', blk)) else -1 for k in FIELDS))
        return out
    def kernels(path):
        lines = open(path).read().split("\n")
        ks, i = {}, 0
        while i < len(lines):
            m = re.match(r"^(_Z\S+):", lines[i])
            if m:
                j = i
                while j < len(lines) and not lines[j].strip().startswith("s_endpgm"): j += 1
                ks[m.group(1)] = lines[i + 1:j + 1]
                i = j
            i += 1
        return ks
    def ops(body):
        return [l.split()[0] for l in (x.strip() for x in body) if l and not l.startswith((";", ".")) and not l.endswith(":")]
    def main_loop(body):
        labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
        best = None
        for i, l in enumerate(body):
            m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.search(r"s_branch\s+(\.LBB\d+_\d+)", l)
            if m and m.group(1) in labels and labels[m.group(1)] < i and (best is None or i - labels[m.group(1)] > best[1] - best[0]):
                best = (labels[m.group(1)], i)
        return body[best[0]:best[1] + 1] if best else []
    WATCH = re.compile(r"k_bwd_fused|k_chunk_walk|k_bwd_lin|k_chunk_walk_lin|k_scan|k_chunk_compose|k_chunk_stitch|k_grid")
    nsym = nd = 0; names_p = set(); names_c = set(); diffres = []; diffasm = []; diffloop = []; same_text = 0; nk = 0
    for tu in tus:
        rp, rc = res(os.path.join(pa, tu, "remarks.txt")), res(os.path.join(ch, tu, "remarks.txt"))
        names_p |= {(tu, n) for n in rp}; names_c |= {(tu, n) for n in rc}
        for n in rp:
            nsym += len(rp[n])
            if n in rc and sorted(rp[n]) != sorted(rc[n]): diffres.append((tu, n, rp[n], rc[n]))
        sp = [f for f in os.listdir(os.path.join(pa, tu)) if f.endswith("gfx950.s")]
        if not sp: continue
        kp, kc = kernels(os.path.join(pa, tu, sp[0])), kernels(os.path.join(ch, tu, sp[0]))
        for k in kp:
            if k not in kc: continue
            nk += 1
            op, oc = ops(kp[k]), ops(kc[k])
            if op == oc: same_text += 1
            else:
                diffasm.append((tu, k, len(op), len(oc)))
                lp, lc = collections.Counter(ops(main_loop(kp[k]))), collections.Counter(ops(main_loop(kc[k])))
                if lp != lc: diffloop.append((tu, k, sum(lp.values()), sum(lc.values()), {o: (lp[o], lc[o]) for o in set(lp) | set(lc) if lp[o] != lc[o]}))
    dm = lambda n: subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()[:150]
    print(f"translation units: {len(tus)} symbols (parent): {nsym}")
    print(f"only in parent: {len(names_p - names_c)} only in change: {len(names_c - names_p)}")
    for t, n in sorted(names_p - names_c): print("  only parent", t, dm(n))
    for t, n in sorted(names_c - names_p): print("  only change", t, dm(n))
    print(f"symbols with differing resources: {len(diffres)}")
    for t, n, a, b in diffres: print("  ", t, dm(n), "\n      parent", a, "\n      change", b)
    print(f"kernels compared by opcode sequence: {nk}, identical: {same_text}, differing: {len(diffasm)}")
    for t, k, a, b in diffasm: print("  ", t, dm(k), f"instructions {a} -> {b}")
    print(f"of them with a differing main-loop histogram: {len(diffloop)}")
    for t, k, a, b, d in diffloop: print("  ", t, dm(k), f"loop {a} -> {b}", d)


if __name__ == "__main__":
    {"build": build, "compare": compare}[sys.argv[1]]()
