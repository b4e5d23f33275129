"""CPU helpers that aim ids at one branch of the binned scatter.

Pass B of the binned scatter (csrc/binned_scatter.hip) keys an LDS hash by
table row: ``hash_slot`` gives a row its home slot, a linear probe of at
most ``PROBE_MAX`` slots wraps at the capacity, a key that finds no slot
gives up and goes through global atomics, and a bin of more than 3/4 of
the capacity skips the hash altogether.  The helpers here compute, in
plain integer arithmetic, which rows share a home, how many updates a bin
gets and how many keys must give up, so that a GPU case can assert on the
CPU that its ids reach the branch it names.

The constants are a copy of the kernel's; ``_C.binned_layout()`` reports
the kernel's own and tests/test_binned_scatter_gpu.py asserts the two
agree.  Everything here runs on the CPU; tests/test_binned_cases.py
covers it.
"""

import torch

HASH_DEEP = 1024        # slots of the dim-16 kernel's hash
HASH_SCALAR = 2048      # slots of the scalar kernel's hash
PROBE_MAX = 64          # probes before a key gives up
HASH_MUL = 2654435761   # hash_slot's multiplier (odd)
LOAD_NUM, LOAD_DEN = 3, 4   # a bin is hashed while count <= 3/4 capacity
J_BITS = 31             # order packs row << J_BITS | update index
SCAN_BLOCK = 1024       # threads of the single-block scan
APPLY_GRID_MAX = 8192   # pass B blocks; more bins are grid-strided
PERM_BLOCK = 256        # count / slot kernels: threads per block ...
PERM_GRID_MAX = 2048    # ... and the most blocks; more ids are strided

# what _C.binned_layout() must report
LAYOUT = {
    "hash_deep": HASH_DEEP,
    "hash_scalar": HASH_SCALAR,
    "hash_max_count_deep": LOAD_NUM * HASH_DEEP // LOAD_DEN,
    "hash_max_count_scalar": LOAD_NUM * HASH_SCALAR // LOAD_DEN,
    "probe_max": PROBE_MAX,
    "hash_mul": HASH_MUL,
    "j_bits": J_BITS,
    "scan_block": SCAN_BLOCK,
    "apply_block": 256,
    "apply_grid_max": APPLY_GRID_MAX,
    "perm_block": PERM_BLOCK,
    "perm_grid_max": PERM_GRID_MAX,
}


def hash_max_count(cap):
    """The largest bin count that still takes the hash."""
    return LOAD_NUM * cap // LOAD_DEN


def home(row, cap):
    """``hash_slot``: the low log2(cap) bits of ``uint32(row) * HASH_MUL``.
    ``row`` is an int or an int64 tensor of rows below 2**31 (the product
    then fits int64; only its low bits are kept anyway).  The multiplier
    is odd, so any ``cap`` consecutive rows map one-to-one onto the slots,
    and rows that agree in their low log2(cap) bits share a home."""
    assert cap & (cap - 1) == 0
    return (row * HASH_MUL) & (cap - 1)


def rows_with_homes(bin_, bits, homes, cap):
    """The rows of region ``bin_`` (``row >> bits == bin_``) whose home is
    in ``homes``, ascending, as an int64 tensor."""
    rows = torch.arange(bin_ << bits, (bin_ + 1) << bits)
    wanted = torch.as_tensor(sorted(set(int(h) % cap for h in homes)))
    return rows[torch.isin(home(rows, cap), wanted)]


def bin_counts(ids, bits, n_rows):
    """Updates per bin, as pass A's histogram must count them."""
    n_bins = (n_rows + (1 << bits) - 1) >> bits
    ids = ids.reshape(-1)
    assert ids.numel() == 0 or (0 <= int(ids.min())
                                and int(ids.max()) < n_rows)
    return torch.bincount(ids >> bits, minlength=n_bins)


def simulate_probe(keys, cap, probe_max=PROBE_MAX):
    """``hash_find_or_insert`` for ``keys`` in the given insertion order,
    into an empty table; returns how many distinct keys give up.  A slot
    once taken stays taken for the bin, so a key's fate is that of its
    first attempt."""
    table = [-1] * cap
    gave_up = set()
    for key in (int(k) for k in keys):
        s = home(key, cap)
        for _ in range(probe_max):
            if table[s] == -1:
                table[s] = key
            if table[s] == key:
                break
            s = (s + 1) & (cap - 1)
        else:
            gave_up.add(key)
    return len(gave_up)


def consecutive_homes(first, count, cap):
    """``count`` consecutive slots from ``first``, wrapping at ``cap``."""
    return [(first + i) % cap for i in range(count)]


def min_give_ups(n_keys, n_homes, probe_max=PROBE_MAX):
    """Keys whose homes are ``n_homes`` consecutive slots reach only
    ``n_homes + probe_max - 1`` slots between them, in any order; the
    rest must give up."""
    return max(0, n_keys - (n_homes + probe_max - 1))
