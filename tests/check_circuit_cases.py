"""The witnesses of the zg_prover_check_circuit tests, as columns of canonical integers, shared by the GPU test
(tests/test_gpu_check_circuit.py) and by the CPU test that holds their reference to its conditions
(tests/test_check_enum_ext_host.py).  Nothing of the library is used here."""
import random

import shuffle_circuits
from check_enum_ext import columns_of
from circuit import R
from shuffle_circuits import BAD

CHUNK = 1024  # row indices per LDS chunk of the device sort

# (circuit, k) of the sort's sizes: below one chunk, exactly one, two chunks (the first global stride), two merge levels
SIZES = [(name, k) for k in (5, 10, 11, 12) for name in ("plain", "wide", "three", "rotated")]
CAPS = (0, 1, 7)  # and total, total + 5


def circuit(name, k=5):
    if name == "wide14":
        return shuffle_circuits.wide(14, high_gate=True)
    if name in ("with_challenge", "with_challenge_phased"):
        return shuffle_circuits.with_challenge(k, name.endswith("phased"))
    return getattr(shuffle_circuits, name)(k)


def challenges_for(pc, seed=1):
    rng = random.Random(7000 + seed)
    return [rng.randrange(R) for _ in pc.challenge_phase]


def cascade(k=5):
    """`only` with ONE shuffle cell moved to the far end of the order (its top limb raised): every position between the
    cell's old place and the end shifts, so about half the rows of the second shuffle fail -- a report longer than any cap
    of CAPS"""
    pc = shuffle_circuits.only(k)
    adv = columns_of(pc, (), 0)
    adv[2][3] = (adv[2][3] + (1 << 224)) % R
    return pc, adv


# ---- adversarial columns for `plain` (a against b, width 1): name -> (k, advice columns)
def plain_cases():
    out = {}
    v = 1 << 100
    for k in (5, 11):
        pc = shuffle_circuits.plain(k)
        n, u = pc.n, pc.usable
        pad = [0] * (n - u)
        r0 = u // 2
        above = [v] * u
        above[r0] = v + 5
        out["one_above_k%d" % k] = (k, [[v] * u + pad, above + pad])  # the single failure: the largest input row, against r0
        below = [v] * u
        below[r0] = v - 5
        out["one_below_k%d" % k] = (k, [[v] * u + pad, below + pad])  # ... row 0, against r0
    pc = shuffle_circuits.plain(11)
    adv = columns_of(pc, (), 0)
    swapped = [list(c) for c in adv]
    swapped[1][CHUNK - 1], swapped[1][CHUNK] = adv[1][CHUNK], adv[1][CHUNK - 1]
    out["swap_across_chunks"] = (11, swapped)  # still a shuffle
    top = [list(c) for c in adv]
    top[1][CHUNK + 7] += 1 << 224
    out["top_limb"] = (11, top)
    low = [list(c) for c in adv]
    low[1][CHUNK + 7] += 1
    out["low_limb"] = (11, low)
    return out


def garbage(pc, adv, seed=5):
    """the same columns with arbitrary values in every row >= usable"""
    rng = random.Random(seed)
    return [list(c[:pc.usable]) + [rng.randrange(R) for _ in range(pc.n - pc.usable)] for c in adv]


# ---- the mixed batch on `three` (columns a, b, c, d, e; lookups on a and c; shuffles a~b, (a,c)~(b,d), c+1~d+1; copy a[0]=e[0])
def mixed_three(k=5):
    pc = shuffle_circuits.three(k)
    good = columns_of(pc, (), 0)
    spoiled = columns_of(pc, (), BAD)
    # a broken copy (e is in the permutation only) and a lookup miss that stays a shuffle: c[5] and the d cell it is
    # shuffled to both leave the table
    broken = [list(c) for c in good]
    broken[4][0] = 4
    s = next(r for r in range(pc.usable) if (good[1][r], good[3][r]) == (good[0][5], good[2][5]))
    broken[2][5] = broken[3][s] = 100
    # every kind the circuit has: the copy, a lookup miss and a spoiled shuffle
    every = [list(c) for c in broken]
    every[3][2] = (every[3][2] + 1) % R
    return pc, [good, spoiled, broken, every]


def mixed_wide(k=5):
    """wide with its gates and lookup: a witness failing a gate, the lookup and the shuffle at once (no permutation)"""
    pc = shuffle_circuits.wide(k, high_gate=True)
    good = columns_of(pc, (), 0)
    bad = columns_of(pc, (), BAD)
    W = shuffle_circuits.MAX_LOOKUP_WIDTH
    bad[2 * W][1] = (bad[2 * W][1] + 1) % R      # p5: the degree-6 gate on row 1
    bad[2 * W + 2][4] = 1000                     # t: no table row holds it
    return pc, [good, bad]
