"""An independent Python restatement of `merge`'s matching rules (pgen_rs_amd/host/merge_match.h), for tests/test_host_merge.py and
the GPU tests of the command.

A table is ``(name, column_line, rows)``: the file's name for messages, its column-header line and its row lines, all without line
ends; a row's file line is taken to be its index + 2 (a file of the column line and the rows) unless ``first_line`` says otherwise."""
from __future__ import annotations


class MergeError(Exception):
    """kind: 'columns' | 'duplicate' | 'pos' | 'iid'; where: the names / line numbers the message must hold."""

    def __init__(self, kind: str, where: tuple):
        super().__init__(f"{kind}: {where}")
        self.kind, self.where = kind, where


def _columns(column_line: str) -> list[str]:
    return column_line.lstrip("#").split("\t") if column_line.startswith("#") else column_line.split("\t")


def match(tables, union: bool = False, first_line: int = 2) -> dict:
    """-> rows: [(from_input, from_row)], src[p][j] (row or -1), flip[p][j], flipped[p], absent[p], dropped[p], id_conflicts"""
    n = len(tables)
    for name, col, _ in tables[1:]:
        if col != tables[0][1]:
            raise MergeError("columns", (tables[0][0], name))
    cols = _columns(tables[0][1])
    c_chrom, c_pos, c_id, c_ref, c_alt = (cols.index(x) for x in ("CHROM", "POS", "ID", "REF", "ALT"))
    found: dict[tuple, dict] = {}   # key -> variant, in first-seen order (dicts keep insertion order)
    chroms: list[str] = []
    for p, (name, _, rows) in enumerate(tables):
        mine = {}
        for r, row in enumerate(rows):
            f = row.split("\t")
            key = (f[c_chrom], f[c_pos], frozenset((f[c_ref], f[c_alt])))
            if union and not (f[c_pos].isascii() and f[c_pos].isdigit()):
                raise MergeError("pos", (name, r + first_line, f[c_pos]))
            if f[c_chrom] not in chroms:
                chroms.append(f[c_chrom])
            if key in mine:
                raise MergeError("duplicate", (name, mine[key] + first_line, r + first_line))
            mine[key] = r
            v = found.setdefault(key, {"first": (p, r), "ref": f[c_ref], "id": f[c_id], "chrom": f[c_chrom], "pos": f[c_pos], "at": {}})
            v["at"][p] = (r, f[c_ref] != v["ref"], f[c_id])
    variants = list(found.values())
    if union:
        variants.sort(key=lambda v: (chroms.index(v["chrom"]), int(v["pos"])))   # stable: ties stay in first-seen order
    else:
        variants = [v for v in variants if len(v["at"]) == n and v["first"][0] == 0]
    out = {"rows": [v["first"] for v in variants], "src": [], "flip": [], "flipped": [], "absent": [], "dropped": [], "id_conflicts": 0}
    for p in range(n):
        src = [v["at"][p][0] if p in v["at"] else -1 for v in variants]
        flip = [int(p in v["at"] and v["at"][p][1]) for v in variants]
        out["src"].append(src)
        out["flip"].append(flip)
        out["flipped"].append(sum(flip))
        out["absent"].append(src.count(-1))
        out["dropped"].append(len(tables[p][2]) - (len(src) - src.count(-1)))
        out["id_conflicts"] += sum(1 for v in variants if p in v["at"] and p != v["first"][0] and v["at"][p][2] != v["id"])
    return out


def check_samples(tables) -> None:
    for name, col, _ in tables[1:]:
        if col != tables[0][1]:
            raise MergeError("columns", (tables[0][0], name))
    c_iid = _columns(tables[0][1]).index("IID")
    seen = {}
    for name, _, rows in tables:
        for row in rows:
            iid = row.split("\t")[c_iid]
            if iid in seen:
                raise MergeError("iid", (iid, seen[iid], name))
            seen[iid] = name


def counts_json(m: dict, n_samples: int) -> dict:
    """What `merge --dry-run` / `--stats` print, timings apart."""
    return {"inputs": len(m["src"]), "samples": n_samples, "variants": len(m["rows"]), "flipped": m["flipped"], "absent": m["absent"],
            "dropped": m["dropped"], "id_conflicts": m["id_conflicts"]}
