"""The table of team kernels, read from the file that defines it, and how a test reaches each of its rows.

rrtplanner_amd/csrc/rrt_block_variants.def is the only list of the instantiated team kernels: `K(G, BSM, PIPE, INF)` one-body
kernels and `S(G, BSM, INF)` committer + worker pairs, dealt to the translation units `RRT_UNIT_k` that `RRT_BLOCK_UNITS`
names.  rrt_engine.hip picks a row at launch time (`plan_launch`, `split_team`, `find_variant`) from the team size, whether
the team is pipelined, whether the launch holds an Informed query, whether the team is the wide one (more than 16 samples per
member) and whether committer and workers run as two kernels.

  rows()            every row of the table, in the file's order
  recipe(row)       what brings a launch to that row through the public C ABI: `Batch` keyword arguments, whether the batch
                    holds an Informed query, and what the near-set radius of its RRT* queries must be
  kernel_name(row)  what rrt_batch_kernel_name prints for it

recipe() restates the conditions of those three functions from the row's side and raises LookupError for a row it has no
rule for: a new kind of row has to come with a way to test it (tests/test_variant_matrix.py runs every row against the
oracle).  Nothing here looks at what a kernel computes.
"""
import collections
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rrtplanner_amd", "csrc")
DEF_PATH = os.path.join(CSRC, "rrt_block_variants.def")
MAKEFILE_PATH = os.path.join(CSRC, "Makefile")

# kind: "K" one kernel, "S" committer + workers as two kernels (always pipelined)
Row = collections.namedtuple("Row", "kind G BSM pipe inf")

# batch: keyword arguments of _ffi.Batch;  informed: the batch holds an Informed query (False: RRTStandard and RRT* only);
# radius: "narrow" = its RRT* queries need r2_rewire < NARROW_R2, "not-narrow" = none of them may have it, None = either
Recipe = collections.namedtuple("Recipe", "batch informed radius")

NARROW_R2 = 257                                   # plan_launch: `d.alg != RRT_ALG_STANDARD && d.r2_rewire < 257u`
TEAMS_UNPIPELINED = (1, 2, 4, 8, 16, 32, 64)      # pick_team: {2, 4, 8, 16, 32, 64}, and one CU per query
TEAMS_PIPELINED = (2, 3, 4, 8, 16, 32, 64)        # pick_team, allow_pipe
SPLIT_FROM = 8                                    # split_team: `team >= 8`
WIDE_TEAM = 2                                     # plan_launch: `p.wide = p.pipe && !inf && p.team == 2 && !narrow`

_BOOL = {"true": True, "false": False}


def _strip_comments(text):
    return "\n".join(line.split("//", 1)[0] for line in text.splitlines())


def parse(text):
    """(units, {unit: [Row, ...]}) of the text of a variants file: the units RRT_BLOCK_UNITS names, in its order, and the
    K / S entries of each unit's RRT_UNIT_k.  Raises ValueError for anything it cannot read as that."""
    text = _strip_comments(text)
    m = re.search(r"^#define\s+RRT_BLOCK_UNITS\(U\)(.*)$", text, re.M)
    if not m:
        raise ValueError("no RRT_BLOCK_UNITS(U) in the variants file")
    units = [int(k) for k in re.findall(r"\bU\((\d+)\)", m.group(1))]
    if not units or len(set(units)) != len(units) or re.sub(r"\bU\(\d+\)", "", m.group(1)).strip():
        raise ValueError(f"RRT_BLOCK_UNITS: {m.group(1).strip()!r}")
    bodies = {int(k): body for k, body in re.findall(r"^#define\s+RRT_UNIT_(\d+)\(K,\s*S\)(.*)$", text, re.M)}
    table = {}
    for k in units:
        if k not in bodies:
            raise ValueError(f"RRT_BLOCK_UNITS names unit {k}, which has no RRT_UNIT_{k}")
        entries = re.findall(r"\b([KS])\(([^()]*)\)", bodies[k])
        if not entries or re.sub(r"\b[KS]\([^()]*\)", "", bodies[k]).strip():
            raise ValueError(f"RRT_UNIT_{k}: {bodies[k].strip()!r}")
        table[k] = []
        for kind, args in entries:
            a = [s.strip() for s in args.split(",")]
            if len(a) != (4 if kind == "K" else 3) or any(s not in _BOOL for s in a[2:]):
                raise ValueError(f"RRT_UNIT_{k}: {kind}({args})")
            flags = [_BOOL[s] for s in a[2:]]
            table[k].append(Row(kind, int(a[0]), int(a[1]), True if kind == "S" else flags[0], flags[-1]))
    unnamed = sorted(set(bodies) - set(units))
    if unnamed:
        raise ValueError(f"RRT_UNIT_{unnamed[0]} is defined and not named in RRT_BLOCK_UNITS")
    return units, table


def _read(path):
    with open(path) as f:
        return f.read()


def units(text=None):
    return parse(_read(DEF_PATH) if text is None else text)[0]


def rows(text=None):
    """every row of the table (of the committed file, or of `text`), unit by unit in the order of RRT_BLOCK_UNITS"""
    us, table = parse(_read(DEF_PATH) if text is None else text)
    return [r for k in us for r in table[k]]


def makefile_units(text=None):
    """the default TUS of the csrc Makefile: every translation unit of kernels_tu.hip the product library is built from"""
    m = re.search(r"^TUS\s*\?=(.*)$", _read(MAKEFILE_PATH) if text is None else text, re.M)
    if not m:
        raise ValueError("no default TUS in the Makefile")
    return [int(k) for k in m.group(1).split()]


def recipe(row):
    wide = row.BSM > 16                                        # find_variant: `(r.BSM > 16) == wide`
    no_rule = LookupError(f"no way known to launch {row}: say in tests/variants.py how plan_launch gets there")
    if row.G not in (TEAMS_PIPELINED if row.pipe else TEAMS_UNPIPELINED):
        raise no_rule                                          # pick_team never forms such a team
    batch = dict(team=row.G, pipe=row.pipe)
    if row.G == 1:
        batch["pipe1"] = False                                 # RRT_FLAG_NOPIPE1: RRTStandard / RRT* would run rrt_pipe_kernel
    if row.kind == "S":                                        # split_team: `pipe && !inf && !wide && team >= 8 && !ONEBODY`
        if row.inf or wide or row.G < SPLIT_FROM:
            raise no_rule
        return Recipe(batch, False, None)
    if wide:                                                   # the wide team: pipelined, two workers, no Informed query
        if not row.pipe or row.inf or row.G != WIDE_TEAM:
            raise no_rule
        return Recipe(batch, False, "not-narrow")
    if row.pipe and not row.inf:
        if row.G >= SPLIT_FROM:
            batch["onebody"] = True                            # RRT_FLAG_ONEBODY: otherwise the S row of this team runs
        elif row.G == WIDE_TEAM:
            return Recipe(batch, False, "narrow")              # otherwise the wide row runs
    return Recipe(batch, row.inf, None)


def _b(v):
    return "true" if v else "false"


def kernel_name(row):
    """rrt_batch_kernel_name in rrt_engine.hip: the snprintf of a row with a committer kernel, and the one of a one-body row"""
    if row.kind == "S":
        return (f"rrt_expand_block_kernel<{row.G}, {row.BSM}, true, {_b(row.inf)}> as rrt_block_commit_kernel + "
                f"rrt_block_work_kernel<{row.G}, {row.BSM}, {_b(row.inf)}>")
    return f"rrt_expand_block_kernel<{row.G}, {row.BSM}, {_b(row.pipe)}, {_b(row.inf)}>"
