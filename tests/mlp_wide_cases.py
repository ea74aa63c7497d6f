"""TEST INFRASTRUCTURE ONLY.  The shapes and input sets of the wide MLP kernels' tests (csrc/mlp_wide_kernels.hip:
hidden 65..128 with obs_dim 32..63), shared by tests/test_mlp_wide_cpu.py -- which checks on the float64 oracle alone
that they are well conditioned -- and the two GPU files.  Inputs come from tests/mlp_oracle.py's case_inputs /
update_inputs with their own seeds."""
import mlp_oracle as O

# (kind, F, H, A): the smallest shapes at which each path of the wide kernels can go wrong
SHAPES = [
    ("chsel", 32, 65, 5),      # both lower edges: the bias in the first column of chunk 1, one row of hidden tile 5
    ("comb", 32, 128, 8),      # uint8 masks, every hidden row used
    ("comb", 46, 128, 16),     # the 16-channel env's widest agent with the default hidden_size; int16 masks
    ("chsel", 47, 80, 9),      # exactly five hidden tiles
    ("comb", 63, 100, 1),      # F + 1 = 64: the bias in the last column; a ragged seventh tile; one action
    ("chsel", 63, 128, 16),    # every upper edge at once
    ("comb", 40, 96, 3),
    ("chsel", 33, 112, 2),
]
SID = lambda s: f"{s[0]}-F{s[1]}-H{s[2]}-A{s[3]}"  # noqa: E731
IDS = [SID(s) for s in SHAPES]
# heterogeneous in_dims at N = 5: agents narrower than 32 columns (chunk 1 holds their bias column only) and one
# of exactly 32
HET = {("comb", 46, 128, 16): [46, 31, 32, 46, 20], ("chsel", 47, 80, 9): [47, 35, 47, 46, 47]}


def batches(shape):
    """(N, E, in_dims) of a shape's policy runs: the E edges are slices of the first"""
    out = [(5, O.E_MAX, None), (1, O.E_MAX, None), (8, O.E_MAX, None), (3, 300, None)]
    if shape in HET:
        out.append((5, O.E_MAX, HET[shape]))
    return out


# ---- the update kernels' input sets
EDGE_SHAPES = [("comb", 46, 128, 16), ("chsel", 32, 65, 5)]
TILE_N = 256
# (shape, T, E, mode) at N = 256: 16-sample tiles per agent = T * ceil(E / 16) = 125 / 75 over 4 waves
TILE_CASES = [
    (("comb", 46, 128, 16), 25, 70, "int"), (("chsel", 32, 65, 5), 75, 9, "int"),
    (("chsel", 32, 65, 5), 25, 70, "mixed"), (("comb", 46, 128, 16), 75, 9, "mixed"),
]
SATURATED = [("comb", 46, 128, 16), ("chsel", 32, 65, 5)]


def update_input_sets():
    """(label, mlp_oracle.update_inputs arguments) of every input set tests/test_mlp_wide_update_gpu.py runs"""
    out = []
    for shape in SHAPES:
        for mode in ("int", "frac"):
            out.append((f"sweep {SID(shape)} {mode}", dict(shape=shape, dims=HET.get(shape), mode=mode, **O.UPD_SWEEP)))
    for shape in EDGE_SHAPES:
        for N in O.UPD_EDGE_N:
            for T, E in O.UPD_TE:
                out.append((f"edge {SID(shape)} N{N} T{T} E{E}", dict(shape=shape, N=N, T=T, E=E)))
    for shape, T, E, mode in TILE_CASES:
        out.append((f"tiles {SID(shape)} T{T} E{E} {mode}", dict(shape=shape, N=TILE_N, T=T, E=E, mode=mode)))
    for shape in SATURATED:
        out.append((f"saturated {SID(shape)}", dict(shape=shape, dims=HET.get(shape), saturated=True, **O.UPD_SWEEP)))
    return out


def wide_blocks(N, n_tiles):
    """The update kernels' grid rule restated (csrc/mlp_wide_kernels.hip wide_blocks): workgroups of 4 waves per
    agent.  Wave w of an agent's 4 G takes the 16-sample tiles w, w + 4 G, ..."""
    G = min((n_tiles + 3) // 4, max(1, 256 // max(1, N)))
    G = max(G, (n_tiles + 1023) // 1024)
    return max(1, min(G, 65535))
