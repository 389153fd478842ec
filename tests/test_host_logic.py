"""Host-side logic of the engine that needs no GPU."""


def test_status_parsers_agree():
    """The engine parses the iteration's status block two ways — from a torch tensor (event path, sharded path) and
    from the NumPy view of the pinned mirror (polled path): same dictionary."""
    import numpy as np
    import torch
    from splat_loam_amd.engine import MappingEngine
    rng = np.random.default_rng(0)
    for flags in (0, 1, 2, 4, 3, 8, 16, 32, 63):
        h = np.zeros(8, np.int32)
        h[0] = np.int32(np.uint32(3_000_000_000).astype(np.int32)) if flags == 1 else 123456      # (R beyond 2^31 too)
        h[1] = flags
        h[2:7] = rng.normal(size=5).astype(np.float32).view(np.int32)
        h[7] = 4242
        a = MappingEngine._parse_status(torch.from_numpy(h.copy()))
        b = MappingEngine._parse_status_np(h.copy())
        assert a == b, (a, b)
        assert a["overflow"] == bool(flags) and a["exchange_count"] == 4242
        bits = [a[k] for k in ("too_small", "resort_failed", "exchange_too_small", "det_mispredicted",
                               "handover_mismatch", "outside_union")]
        assert bits == [bool(flags & (1 << i)) for i in range(6)], (flags, a)
        assert a["R"] == (3_000_000_000 if flags == 1 else 123456)
        f = h[2:7].view(np.float32)
        assert a["sums"] == [float(f[0]), float(f[1]), float(f[2])] and a["loss"] == float(f[3]) + float(f[4])


def test_repair_rounds_table():
    """engine.repair_rounds against values worked out by hand from the rule it replaced in the engine's order lookup:
    0 unless reuse is allowed, the order has an age and that age is <= max_order_age_extra; else
    min(base + [age > max_order_age] + [age > order_age_round3] + [age > order_age_round4], 4)."""
    from splat_loam_amd.engine import repair_rounds
    ages = (4, 12, 48, 1000000)         # max_order_age, order_age_round3, max_order_age_extra, order_age_round4
    #        age:  None  0  4  5  12  13  48  49  1000000  1000001
    table = {1: (0,    1, 1, 2, 2,  3,  3,  0,  0,       0),
             2: (0,    2, 2, 3, 3,  4,  4,  0,  0,       0),
             3: (0,    3, 3, 4, 4,  4,  4,  0,  0,       0)}        # (3 + 2 = 5: capped at 4)
    for base, want in table.items():
        for age, w in zip((None, 0, 4, 5, 12, 13, 48, 49, 1000000, 1000001), want):
            got = repair_rounds(age, base, *ages, True)
            assert got == w and isinstance(got, int), (age, base, got, w)
            assert repair_rounds(age, base, *ages, False) == 0, (age, base)
    # a fourth-round age below the rebuild age: the third increment, and the cap with it
    ages = (4, 12, 48, 30)
    #        age:  30 31 48 49
    table = {1: (3, 4, 4, 0),
             2: (4, 4, 4, 0),           # (31: 2 + 3 = 5, capped)
             3: (4, 4, 4, 0)}           # (30: 3 + 2 = 5, 31: 3 + 3 = 6, capped)
    for base, want in table.items():
        for age, w in zip((30, 31, 48, 49), want):
            assert repair_rounds(age, base, *ages, True) == w, (age, base)
            assert repair_rounds(age, base, *ages, False) == 0, (age, base)
