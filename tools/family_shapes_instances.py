"""Which kernel instances the cases of tests/_family_shapes.py launch, without a GPU: every case's entry points (the calls of
tests/test_gpu_family_shapes.py, numbers ignored) against a library linked with tools/hip_recorder.cpp, which runs no kernel and
logs every launch by name.  The recording library is built from the objects of a normal build
(make -C gaussian_process_optimization_amd/csrc) in a copy of the package outside the tree, as the header of hip_recorder.cpp
describes; each case runs in a process of its own.
usage: family_shapes_instances.py [out.txt]        (default: profiles/family_shapes_instances.txt)
       family_shapes_instances.py --case <family> <case id>      (one case, inside the recording build: what the driver starts)"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "gaussian_process_optimization_amd"
sys.path += [os.path.join(ROOT, "tests"), ROOT]   # (behind PYTHONPATH: a case imports the recording copy of the package)
import _family_shapes as FS   # noqa: E402

TILE_KERNELS = ("kbuild_kernel", "kbuild_batch_kernel", "cross_k_kernel")
GRAD_KERNELS = ("lml_grad_tile_kernel", "lml_grad_tile_batch_kernel")
SHOWN = re.compile(r"^(kbuild|cross_k|lml_grad|predict_grad|rows_)")


def run_case(fam, cid):
    """The entry points of one case, in the order of the GPU tests."""
    import numpy as np
    from gaussian_process_optimization_amd import _lib
    c = FS.CASES[cid]
    X, Y, Xs, ls = FS.problem(cid)
    kid, EI = FS.KERNEL_ID[fam], _lib.GP_ACQ_EI
    h = _lib.Handle(0)
    h.set_option("emulate_fp64", 0)
    h.set_data(X, Y)
    h.set_params(kid, int(c.ard), FS.VAR, ls, FS.NOISE)
    h.kernel_matrix()
    h.cross_kernel_matrix(Xs)
    h.fit()
    h.lml_grad(ls.size)
    h.fit_grad(ls.size)
    h.set_candidates(Xs)
    h.predict(True)
    h.fit_predict(True)
    h.predict_full_cov(True)
    h.predict_grad()
    h.predict_grad(mean_only=True)
    if c.P == 1:
        fmin = h.fmin()
        for t, par in ((_lib.GP_ACQ_EI, 0.01), (_lib.GP_ACQ_LCB, 2.0), (_lib.GP_ACQ_MPI, 0.01)):
            h.acq(t, par, fmin)
            h.acq_grad(t, par, fmin)
            h.acq_argbest(t, par, fmin, -1)
        for k in FS.rows_counts(c):
            x = np.array(FS.rows_points(cid)[:k])
            s0 = h.rows_stats()
            h.predict_rows(x, True, grad=True)
            h.acq_rows(x, EI, 0.01, fmin, grad=True)
            h.mean_grad_rows(x)
            s1 = h.rows_stats()
            fused = FS.rows_fused(k, c.D)
            assert s1["fused"] - s0["fused"] == (3 if fused else 0) and s1["fallback"] - s0["fallback"] == (0 if fused else 3), (k, s0, s1)
    if (fam, cid) in FS.BATCH:
        h.set_data(X, Y)
        h.set_params(kid, int(c.ard), FS.VAR, ls, FS.NOISE)
        status = h.fit_grad_batch(*FS.members(cid))[2]
        assert not status.any()
    h.close()


def build_recording_copy(work):
    csrc = os.path.join(ROOT, PKG, "csrc")
    if not glob.glob(os.path.join(csrc, "*.o")):
        subprocess.check_call(["make", "-C", csrc, "-j", "6"])
    pkg = os.path.join(work, PKG)
    os.makedirs(pkg)
    for f in glob.glob(os.path.join(ROOT, PKG, "*.py")):
        shutil.copy(f, pkg)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    obj = os.path.join(work, "hip_recorder.o")
    subprocess.check_call(["g++", "-O1", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include", "-c",
                           os.path.join(ROOT, "tools", "hip_recorder.cpp"), "-o", obj])
    subprocess.check_call(["g++", "-shared", "-fPIC"] + sorted(glob.glob(os.path.join(csrc, "*.o"))) + [obj, "-o", os.path.join(pkg, "libgphip.so")])


def demangle(names):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    tool = shutil.which("c++filt") or os.path.join(rocm, "llvm", "bin", "llvm-cxxfilt")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for m, d in zip(names, out):
        d = re.sub(r"^void ", "", d)
        depth, end = 0, len(d)
        for i, ch in enumerate(d):          # cut the parameter list: the first "(" outside the template arguments
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                end = i
                break
        short[m] = d[:end]
    return short


def launched(log):
    with open(log) as f:
        return [(w[1], w[3]) for w in (line.split() for line in f if line.startswith("launch "))]   # (mangled name, grid x,y,z)


def main(out_path):
    work = tempfile.mkdtemp(prefix="family_shapes_rec_")
    try:
        build_recording_copy(work)
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([work, os.path.join(ROOT, "tests"), ROOT]), PYTHONDONTWRITEBYTECODE="1")
        per_case, left_out = {}, []
        for fam, cid in FS.SINGLE:
            log = os.path.join(work, "%s-%s.log" % (fam, cid))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", fam, cid], env=dict(env, HIP_RECORDER_LOG=log),
                               cwd=work, capture_output=True, text=True)
            if p.returncode:
                left_out.append((fam, cid, (p.stderr.strip().split("\n") or ["?"])[-1]))
                continue
            per_case[(fam, cid)] = launched(log)
        short = demangle(sorted({n for names in per_case.values() for n, _ in names}))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    lines = ["Kernel instances launched by the cases of tests/_family_shapes.py (no GPU: tools/hip_recorder.cpp)",
             "=" * 98, "",
             "How: python tools/family_shapes_instances.py -- the entry points of every (family, case) of tests/test_gpu_family_shapes.py",
             "(matrices, fit, gradients, prediction, acquisitions, one-location calls with their route counters checked, and",
             "gp_fit_grad_batch where the case is in the batch list) against a library linked with the recorder; per case, the distinct",
             "kbuild*, cross_k*, lml_grad*, predict_grad and rows_* kernels in order of first launch, with launch counts.  (The recorder", "carried every case: none is left out.)" if not left_out else "", ""]
    reached = {}
    for (fam, cid), names in per_case.items():
        c = FS.CASES[cid]
        lines.append("%s-%s  N = %d, D = %d, M = %d, P = %d, %s, offset %g: %s" % (fam, cid, c.N, c.D, c.M, c.P, "ARD" if c.ard else "iso", c.off, c.reaches))
        seen = {}
        for n, grid in names:
            s = short[n]
            if SHOWN.match(s):   # the gradient tile kernels with their grid: lower tiles, split (4 below 256 tiles, else 1), members
                key = (s, "   grid %s" % grid if s.startswith("lml_grad") else "")
                seen[key] = seen.get(key, 0) + 1
        for (s, grid), k in seen.items():
            lines.append("    %-44s x %-3d%s" % (s, k, grid))
            reached.setdefault((s, fam in FS.NEW_FAMILIES), []).append(cid)
        lines.append("")
    for fam, cid, why in left_out:
        lines.append("%s-%s  LEFT OUT: the recorder could not carry this case (%s)" % (fam, cid, why))
    lines += ["Instances of the tile kernels and of the gradient kernels: the Matern-3/2 / Exponential cases that launch them, and",
              "[in brackets] the rbf / Mat52 cases (pair 0 at D <= 16 is the business of the rest of the suite)", "-" * 98]
    inst = ["%s<%d, %d>" % (k, du, fp) for k in TILE_KERNELS for du in (8, 16, 0) for fp in (0, 1)] + ["%s<%d>" % (k, fp) for k in GRAD_KERNELS for fp in (0, 1)]
    missing = []
    for s in inst:
        cases, old = sorted(set(reached.get((s, True), []))), sorted(set(reached.get((s, False), [])))
        pair1 = s.endswith("1>")
        lines.append("  %-36s %-8s %s%s" % (s, "reached" if cases else ("-" if not pair1 else "MISSING"), " ".join(cases),
                                             "[%s]" % " ".join(old) if old else ""))
        if pair1 and not cases:
            missing.append(s)
    lines += ["", "pair-1 instances not reached: %d" % len(missing)]
    with open(out_path, "w") as f:
        f.write("\n".join(line.rstrip() for line in lines) + "\n")
    print("\n".join(lines[-(len(inst) + 3):]))
    return 1 if missing else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--case":
        run_case(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "family_shapes_instances.txt")))
