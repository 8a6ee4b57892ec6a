"""profiles/output_limits.txt from the lines tests/test_gpu_output_limits.py prints:

    python -m pytest tests/test_gpu_output_limits.py -m gpu -q -s > log.txt
    python tools/output_limits_table.py log.txt > profiles/output_limits.txt

Every "output_limits: <case> <quantity> <error> tol <bound>" line is the device against the float64 oracle at the limits of the
output count P and the input dimension D (tests/_output_limits.py), per output column where the quantity has one; the table is
the maximum per case and quantity group, followed by the worst figure of every group and where it was measured.  The bounds the
test asserts: lml 1e-8, logdet 1e-10, everything else 1e-6.
"""
import collections
import re
import sys

LINE = re.compile(r"output_limits:\s+(\S+)\s+(.+?)\s+(\d\.\d+e[+-]\d+)\s+tol")
# quantity -> column: the routes (tile / small-M), the batch members and the three gradient entries share a column
GROUPS = (("lml", "lml"), ("logdet", "logdet"), ("alpha", "alpha"), ("woodbury", "alpha"), ("mean", "mean"), ("var", "var"),
          ("full_cov", "full_cov"), ("dmdx", "dmdx"), ("dvdx", "dvdx"), ("dL_dX", "dL_dX"), ("dZ", "dZ"))
ORDER = ["lml", "logdet", "alpha", "mean", "var", "full_cov", "dmdx", "dvdx", "grad", "dL_dX", "dZ"]


def group(q):
    if q.endswith((" dvariance", " dlengthscale", " dnoise")):
        return "grad"
    if q.endswith(" lml"):
        return "lml"
    if q == "full_cov mean":
        return "mean"
    for head, g in GROUPS:
        if q.startswith(head):
            return g
    return q.split()[0]


def main(path):
    rows, worst, n = collections.OrderedDict(), {}, 0
    for line in open(path):
        m = LINE.search(line)
        if not m:
            continue
        case, q, v = m.group(1), m.group(2), float(m.group(3))
        g = group(q)
        n += 1
        d = rows.setdefault(case, {})
        d[g] = max(d.get(g, 0.0), v)
        if v >= worst.get(g, (-1.0,))[0]:
            worst[g] = (v, case, q)
    print("tests/test_gpu_output_limits.py on one MI355X: device against the float64 oracle, maxima over %d lines" % n)
    print("(per output column, relative to the column's largest reference entry, where the quantity has columns; alpha also holds")
    print("the sparse model's woodbury vector and inverse, mean / var both candidate routes and both noise settings, grad the")
    print("hyper-parameter gradients of gp_lml_grad, gp_fit_grad, the three members of gp_fit_grad_batch and gp_sparse_fit_grad;")
    print("the look-ahead routes are bitwise the single-stream rows rbf-LA-W1 / -W2 and have no line of their own)")
    print()
    print(("%-22s %s" % ("case", " ".join("%-9s" % k for k in ORDER))).rstrip())
    for c, d in rows.items():
        print(("%-22s %s" % (c, " ".join("%-9s" % ("%.1e" % d[k] if k in d else "-") for k in ORDER))).rstrip())
    print()
    print("worst per quantity:")
    for k in ORDER:
        if k in worst:
            print("  %-9s %.1e  %s, %s" % (k, worst[k][0], worst[k][1], worst[k][2]))
    print("worst of all: %.1e" % max(v[0] for v in worst.values()))


if __name__ == "__main__":
    main(sys.argv[1])
