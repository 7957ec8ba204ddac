"""gen_db_term_table.py -- writes hpfw_amd/csrc/db_tab.h, the constants of db_term_fast (db_spec.h):
per cell i of the mantissa interval [1, 2) the pair (1 / c_i, 10 log10(c_i)) with c_i the cell's centre, the scaled
coefficients of log1p's series, and 10 log10(2).  Every value is rounded once from 60 decimal digits and written as a
hex float, so the header does not depend on the libm of the machine that ran this.  What the values are is not what
makes db_term_fast right: tests/emu/db_term_check.cpp compares it with db_term_spec on every input.

  python tools/gen_db_term_table.py [log2 of the cell count, default 6] [degree, default 5]
"""
import os
import sys
from decimal import Decimal, getcontext
from fractions import Fraction

getcontext().prec = 60
bits = int(sys.argv[1]) if len(sys.argv) > 1 else 6
degree = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cells = 1 << bits
ln10 = Decimal(10).ln()
k = Decimal(10) / ln10


def hexf(d):
    return float(d).hex()


lines = [
    "// db_tab.h -- written by tools/gen_db_term_table.py %d %d; do not edit.  The constants of db_term_fast (db_spec.h)." % (bits, degree),
    "#pragma once",
    "#define HPFW_DB_CELL_BITS %d" % bits,
    "#define HPFW_DB_DEGREE %d" % degree,
    "// 10 log10(2)",
    "#define HPFW_DB_LOG2 %s" % hexf(Decimal(10) * Decimal(2).log10()),
    "// (-1)^(k+1) (10 / ln 10) / k, k = 1 .. degree: 10 log10(1 + r) = sum of these times r^k",
    "#define HPFW_DB_POLY { " + ", ".join(hexf((k if j % 2 else -k) / j) for j in range(1, degree + 1)) + " }",
    "// cell i: { 1 / c_i, 10 log10(c_i) }, c_i = 1 + (i + 1/2) / %d" % cells,
    "#define HPFW_DB_TABLE { \\",
]
for i in range(cells):
    c = Fraction(2 * cells + 2 * i + 1, 2 * cells)
    cd = Decimal(c.numerator) / Decimal(c.denominator)
    lines.append("    { %s, %s }, \\" % (float(1 / c).hex(), hexf(Decimal(10) * cd.log10())))
lines.append("}")
out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpfw_amd", "csrc", "db_tab.h")
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(out, cells, "cells, degree", degree)
