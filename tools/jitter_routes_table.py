"""profiles/jitter_routes.txt from the lines tests/test_gpu_jitter_routes.py prints:

    python -m pytest tests/test_gpu_jitter_routes.py -m gpu -q -s > log.txt
    python tools/jitter_routes_table.py log.txt > profiles/jitter_routes.txt

Every "jitter_routes: <route> <case ...> <quantity> <error> ..." line is the device against the float64 oracle on inputs whose fit
needs the jitter ladder (tests/_jitter_cases.py); the table is the maximum per route and quantity, followed by where each
maximum above 1e-10 was measured.  The bounds the test asserts: jitter 1e-12, lml and logdet 1e-8, ei_grad 1e-5, var0 1e-6 + 1e-9
absolute, everything else 1e-6.
"""
import collections
import re
import sys

ORDER = ["jitter", "lml", "logdet", "alpha", "mean", "var", "mean0", "var0", "full_cov", "Wi", "lml_grad", "dmean", "dvar", "rows",
         "rows_grad", "ei", "ei_grad", "fmin", "fmin_direct"]


def main(path):
    rows, where, n = collections.OrderedDict(), {}, 0
    for line in open(path):
        i = line.find("jitter_routes:")
        if i < 0:
            continue
        body = line[i + len("jitter_routes:"):].rstrip("\n")
        pairs = re.findall(r"(\w+) (\d\.\de[+-]\d+)", body)
        tag = body[:body.find(pairs[0][0] + " " + pairs[0][1])].strip()
        route = tag.split()[0]
        d = rows.setdefault(route, {})
        n += 1
        for k, v in pairs:
            if float(v) >= d.get(k, -1.0):
                d[k] = float(v)
                where[route, k] = tag
    print("tests/test_gpu_jitter_routes.py on one MI355X: device against the float64 oracle under jitter, maxima over %d lines" % n)
    print("(single-W*: lookahead = 0, every row and delta of tests/_jitter_cases.py; inner2-* / emulated-*: the ten-tile rows at")
    print("delta = 3e-5 through gp_fit, gp_fit_predict and gp_fit_grad; append / border: gp_append on and after jittered fits;")
    print("the fp64 look-ahead routes are bitwise single-W1 / single-W3 and have no line of their own)")
    print()
    print(("%-18s %s" % ("route", " ".join("%-9s" % k for k in ORDER))).rstrip())
    for r, d in rows.items():
        print(("%-18s %s" % (r, " ".join("%-9s" % ("%.1e" % d[k] if k in d else "-") for k in ORDER))).rstrip())
    print()
    print("where each maximum above 1e-10 was measured:")
    for (r, k), tag in where.items():
        if rows[r][k] > 1e-10:
            print("  %-18s %-9s %.1e  %s" % (r, k, rows[r][k], tag))


if __name__ == "__main__":
    main(sys.argv[1])
