"""The switch table of INTEGRATION.md section 6 names exactly the GSA_* variables the library reads."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names_read_by_the_sources():
    names = set()
    csrc = os.path.join(ROOT, "gan-segmentation_amd", "csrc")
    for path in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")):
        with open(path) as f:
            names.update(re.findall(r'\b(?:env_int|getenv)\(\s*"(GSA_[A-Z0-9_]+)"', f.read()))
    return names


def _names_in_the_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        rows = [line.strip() for line in f if line.strip().startswith("|")]
    head = next(i for i, row in enumerate(rows) if row.startswith("| name | default | build |"))
    names = []
    for row in rows[head + 2:]:
        m = re.match(r"\| `(GSA_[A-Z0-9_]+)` \|", row)
        if not m:
            break
        names.append(m.group(1))
    return names


def test_switch_table_lists_every_variable_the_sources_read():
    """Every name passed to env_int (gsa_kernels.h; GSA_VERBOSE, a presence test, goes to getenv itself) in csrc/*.hip and
    csrc/*.cpp has a row in the table, every row names a variable the sources read, and no name has two rows."""
    read, table = _names_read_by_the_sources(), _names_in_the_table()
    assert len(read) > 30, "the scan of the sources found too few names: %r" % sorted(read)
    assert len(table) == len(set(table)), "rows twice in the table: %r" % sorted(n for n in set(table) if table.count(n) > 1)
    assert set(table) == read, "only in the sources: %r; only in the table: %r" % (sorted(read - set(table)), sorted(set(table) - read))
