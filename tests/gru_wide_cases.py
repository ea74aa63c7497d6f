"""TEST INFRASTRUCTURE ONLY.  The input sets of the wide GRU kernels' tests (csrc/gru_wide_kernels.hip: hidden sizes
65..128): tests/test_gru_wide_cpu.py asserts on the CPU the conditions that let tests/test_gru_wide_gpu.py hold every
sample to the strict tolerances, exactly as tests/test_gru_oracle_cpu.py does for tests/test_gru_edges_gpu.py.

The sets are gru_oracle.Case tuples built by gru_oracle.case (N = 2 agents, E = 17 envs: a full 16-env tile and a tile
of one env, 3-step windows unless the set is about the window) with the seed bump of BUMP below: for each set the first
bump >= 0 at which the conditions hold (no ambiguous head-relu pair, every probability in [1e-3, 1 - 1e-3], torch fp32
autograd within the gradient tolerance, no clip edge within 5e-4).  The wider the head, the likelier one of its
H x samples pre-activations falls within fp32 rounding of zero, so every set with H >= 96 has one 5-slot episode
(T = 5, 170 windows) where the narrow file has two; H = 65, 72 and 80 keep T = 10."""
import gru_oracle as O

KINDS = O.KINDS

# cid -> the first seed bump that meets the conditions of test_gru_wide_cpu.py::test_input_set_conditions (sets not
# listed: bump 0).  Found by running those conditions over bumps 0, 1, 2, ... on the CPU.
BUMP = {
    'sigmoid-F12-H100-A8-L3-ep5-T5-E17-N2-all': 2,
    'sigmoid-F12-H100-A8-L3-ep5-T5-E17-N2-column': 3,
    'sigmoid-F15-H128-A8-L3-ep5-T5-E17-N2': 3,
    'sigmoid-F15-H65-A8-L3-ep5-T10-E17-N2': 3,
    'sigmoid-F30-H100-A1-L3-ep5-T5-E17-N2': 4,
    'sigmoid-F30-H100-A2-L3-ep5-T5-E17-N2': 1,
    'sigmoid-F30-H100-A8-L1-ep5-T5-E17-N2': 1,
    'sigmoid-F30-H100-A8-L3-ep5-T5-E33-N2': 69,
    'sigmoid-F30-H100-A8-L65-ep6-T6-E3-N2': 1,
    'sigmoid-F30-H100-A8-L8-ep5-T5-E17-N2': 6,
    'sigmoid-F30-H113-A8-L3-ep5-T5-E17-N2': 6,
    'sigmoid-F30-H96-A8-L3-ep5-T5-E17-N2': 4,
    'sigmoid-F31-H128-A8-L3-ep5-T5-E17-N2': 8,
    'sigmoid-F31-H80-A8-L3-ep5-T10-E17-N2': 5,
    'sigmoid-F40-H100-A8-L3-ep5-T5-E17-N2-all': 4,
    'sigmoid-F40-H100-A8-L3-ep5-T5-E17-N2-one': 8,
    'sigmoid-F46-H128-A8-L3-ep5-T5-E17-N2-d46_39': 26,
    'sigmoid-F47-H128-A8-L3-ep5-T5-E17-N2': 8,
    'sigmoid-F63-H128-A8-L3-ep5-T5-E17-N2': 38,
    'sigmoid-F63-H65-A8-L3-ep5-T10-E17-N2': 1,
    'softmax-F12-H100-A5-L3-ep5-T5-E17-N2-all': 3,
    'softmax-F12-H100-A5-L3-ep5-T5-E17-N2-column': 7,
    'softmax-F12-H100-A5-L3-ep5-T5-E17-N2-one': 10,
    'softmax-F15-H128-A5-L3-ep5-T5-E17-N2': 3,
    'softmax-F15-H72-A5-L3-ep5-T10-E17-N2': 1,
    'softmax-F30-H100-A16-L3-ep5-T5-E17-N2': 5,
    'softmax-F30-H100-A2-L3-ep5-T5-E17-N2': 18,
    'softmax-F30-H100-A5-L1-ep5-T5-E17-N2': 2,
    'softmax-F30-H100-A5-L3-ep5-T5-E17-N2': 6,
    'softmax-F30-H100-A5-L3-ep5-T5-E17-N2-d30_22': 9,
    'softmax-F30-H100-A5-L3-ep5-T5-E33-N2': 11,
    'softmax-F30-H100-A5-L64-ep6-T6-E3-N2': 2,
    'softmax-F30-H100-A5-L65-ep6-T6-E3-N2': 1,
    'softmax-F30-H100-A5-L8-ep5-T5-E17-N2': 21,
    'softmax-F30-H127-A5-L3-ep5-T5-E17-N2': 4,
    'softmax-F31-H128-A5-L3-ep5-T5-E17-N2': 24,
    'softmax-F31-H65-A5-L3-ep5-T10-E17-N2': 1,
    'softmax-F40-H100-A5-L3-ep5-T5-E17-N2-column': 4,
    'softmax-F47-H128-A5-L3-ep5-T5-E17-N2': 8,
    'softmax-F47-H80-A5-L3-ep5-T10-E17-N2': 1,
    'softmax-F63-H128-A5-L3-ep5-T5-E17-N2': 16,
    'softmax-F63-H72-A5-L3-ep5-T10-E17-N2': 2,
    'value-F12-H100-A1-L3-ep5-T5-E17-N2-all': 3,
    'value-F12-H100-A1-L3-ep5-T5-E17-N2-column': 2,
    'value-F12-H100-A1-L3-ep5-T5-E17-N2-one': 5,
    'value-F15-H128-A1-L3-ep5-T5-E17-N2': 2,
    'value-F15-H80-A1-L3-ep5-T10-E17-N2': 13,
    'value-F30-H100-A1-L1-ep5-T5-E17-N2': 6,
    'value-F30-H100-A1-L3-ep5-T5-E17-N2': 1,
    'value-F30-H100-A1-L3-ep5-T5-E33-N2': 39,
    'value-F30-H112-A1-L3-ep5-T5-E17-N2': 24,
    'value-F31-H128-A1-L3-ep5-T5-E17-N2': 43,
    'value-F31-H72-A1-L3-ep5-T10-E17-N2': 8,
    'value-F40-H100-A1-L3-ep5-T5-E17-N2-all': 10,
    'value-F40-H100-A1-L3-ep5-T5-E17-N2-column': 1,
    'value-F40-H100-A1-L3-ep5-T5-E17-N2-one': 13,
    'value-F47-H128-A1-L3-ep5-T5-E17-N2': 5,
    'value-F63-H128-A1-L3-ep5-T5-E17-N2': 18,
    'value-F63-H80-A1-L3-ep5-T10-E17-N2': 5,
}


def case(kind, F, H, **kw):
    if H >= 96 and "T" not in kw:
        kw["T"] = kw.get("ep", 5)
    c = O.case(kind, F, H, **kw)
    return c._replace(bump=BUMP.get(O.cid(c), 0))


def tiles(c):
    """(HT, IT): the kernels' run-time hidden and input tile counts (no bias column on this path)"""
    return (c.H + 15) // 16, (c.F + 15) // 16


# (1) H = 128 (HT = 8, every row real) at IT = 1 .. 4
MATRIX = [case(k, F, 128) for F in (15, 31, 47, 63) for k in KINDS]
# (2) ragged hidden sizes (HT = 6 .. 8; 100 is the RNN module's default), kinds rotating, and H = 100 for all kinds
RAGGED_H = [case(KINDS[i % 3], 30, H) for i, H in enumerate((96, 100, 112, 113, 127))]
BASE_CASES = [case(k, 30, 100) for k in KINDS]
RAGGED_A = [case("sigmoid", 30, 100, A=A) for A in (1, 2, 9)] + [case("softmax", 30, 100, A=A) for A in (2, 16)]
RAGGED_DIMS = [case("sigmoid", 46, 128, dims=(46, 39)), case("softmax", 30, 100, dims=(30, 22))]
RAGGED_E = [case(None, 30, 100, E=16)]
# (3) fractional inputs (fp32 rows only): every product is exact fp32 here, so these hold to the same tolerance
FRAC = [case(k, F, 100, frac=fr) for F in (12, 40) for k in KINDS for fr in O.FRAC_MODES[1:]]
# (4) the low end of the envelope: HT = 5 with 1, 8 and 16 of its 16 units, at every IT, kinds rotating
LOW = [case(KINDS[(i + j) % 3], F, H) for i, H in enumerate((65, 72, 80)) for j, F in enumerate((15, 31, 47, 63))]
# (5) windows: L > episode, L = 1, and the long windows (one episode of 6 slots at E = 3: the reference's cost)
WINDOW_MISC = [case(k, 30, 100, L=L) for L in (8, 1) for k in KINDS]
WINDOW_LONG = [case(k, 30, 100, L=L, ep=6, T=6, E=3) for L in (64, 65) for k in KINDS]
# (6) three env tiles per slot, 15 tiles per agent: the update in one chunk and in fifteen
CHUNK = [case(k, 30, 100, E=33) for k in KINDS]


def all_cases():
    seen, out = set(), []
    for c in MATRIX + RAGGED_H + BASE_CASES + RAGGED_A + RAGGED_DIMS + RAGGED_E + FRAC + LOW + WINDOW_MISC + WINDOW_LONG + CHUNK:
        if O.cid(c) not in seen:
            seen.add(O.cid(c))
            out.append(c)
    return out


def exact(cases):
    """the sets whose inputs are integers: the compact record holds them"""
    return [c for c in cases if c.frac == "none"]
