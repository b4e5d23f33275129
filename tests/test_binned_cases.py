"""CPU tests of tests/binned_cases.py: the bijection of the home slots and
the two facts about the probe that the GPU cases of
tests/test_binned_scatter_gpu.py rest on."""

import pytest
import torch

import binned_cases as bc

CAPS = (bc.HASH_DEEP, bc.HASH_SCALAR)
BITS = 14  # the widest region pick_region_bits chooses


def test_home_matches_uint32_arithmetic():
    for row in (0, 1, 1023, 1024, 2 ** 20 + 7, 2 ** 31 - 1):
        for cap in CAPS:
            want = ((row * 2654435761) % 2 ** 32) % cap
            assert bc.home(row, cap) == want
            assert int(bc.home(torch.tensor([row]), cap)) == want


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("first", [0, 5, 16384, 2 ** 31 - 2048])
def test_home_is_a_bijection_on_consecutive_rows(cap, first):
    homes = bc.home(torch.arange(first, first + cap), cap)
    assert torch.equal(homes.sort().values, torch.arange(cap))
    # rows that agree in their low log2(cap) bits share a home
    assert bc.home(first + 3, cap) == bc.home(first + 3 + 5 * cap, cap)


@pytest.mark.parametrize("cap", CAPS)
def test_rows_with_homes(cap):
    homes = bc.consecutive_homes(cap - 2, 4, cap)
    assert homes == [cap - 2, cap - 1, 0, 1]
    rows = bc.rows_with_homes(1, BITS, homes, cap)
    assert rows.numel() == 4 * (2 ** BITS // cap)
    assert torch.equal(rows >> BITS, torch.ones_like(rows))
    assert set(bc.home(rows, cap).tolist()) == set(homes)
    others = bc.rows_with_homes(1, BITS, [7], cap)
    assert others.numel() == 2 ** BITS // cap
    assert not set(others.tolist()) & set(rows.tolist())


def test_bin_counts():
    ids = torch.tensor([0, 1, 2, 3, 8, 8, 8, 20])
    assert bc.bin_counts(ids, 2, 21).tolist() == [4, 0, 3, 0, 0, 1]
    assert bc.bin_counts(ids[:0], 2, 21).tolist() == [0] * 6
    with pytest.raises(AssertionError):
        bc.bin_counts(ids, 2, 20)


def test_simulate_probe_small():
    cap = 8
    same_home = [k for k in range(64) if bc.home(k, cap) == 3][:4]
    assert bc.simulate_probe(same_home, cap, probe_max=4) == 0
    assert bc.simulate_probe(same_home, cap, probe_max=3) == 1
    # a repeated key finds its own slot again
    assert bc.simulate_probe(same_home * 2, cap, probe_max=4) == 0
    assert bc.simulate_probe(same_home * 2, cap, probe_max=3) == 1


def _orders(keys, n_orders, seed):
    gen = torch.Generator().manual_seed(seed)
    for _ in range(n_orders):
        yield keys[torch.randperm(keys.numel(), generator=gen)].tolist()


@pytest.mark.parametrize("cap,n_homes", [
    (bc.HASH_DEEP, 4), (bc.HASH_DEEP, 8), (bc.HASH_DEEP, 64),
    (bc.HASH_SCALAR, 8), (bc.HASH_SCALAR, 16), (bc.HASH_SCALAR, 64)])
def test_probe_max_keys_never_give_up(cap, n_homes):
    """At most PROBE_MAX distinct keys in a bin: a probing key meets at
    most PROBE_MAX - 1 slots taken by others, so it finds an empty slot or
    its own within PROBE_MAX probes, in any order.  The homes straddle the
    end of the table, so every cluster wraps (test_simulate_probe_small
    shows the bound is sharp: one key more can give up)."""
    homes = bc.consecutive_homes(cap - n_homes // 2, n_homes, cap)
    keys = bc.rows_with_homes(1, BITS, homes, cap)
    per_home = bc.PROBE_MAX // n_homes
    keys = torch.cat([keys[bc.home(keys, cap) == h][:per_home]
                      for h in homes])
    assert keys.numel() == bc.PROBE_MAX
    for order in _orders(keys, 50, seed=cap + n_homes):
        assert bc.simulate_probe(order, cap) == 0


# (capacity, homes, rows per home, keys that must give up)
GIVE_UP_SETS = [(bc.HASH_DEEP, 8, 16, 57), (bc.HASH_SCALAR, 16, 8, 49)]


@pytest.mark.parametrize("where", ["mid", "wrap"])
@pytest.mark.parametrize("cap,n_homes,per_home,must", GIVE_UP_SETS)
def test_crowded_homes_give_up_in_every_order(cap, n_homes, per_home,
                                              must, where):
    """128 keys on n_homes consecutive homes reach n_homes + 63 slots, so
    at least ``must`` of them give up whatever the order."""
    first = cap // 2 if where == "mid" else cap - n_homes // 2
    keys = bc.rows_with_homes(1, BITS, bc.consecutive_homes(
        first, n_homes, cap), cap)
    assert keys.numel() == n_homes * per_home == 128
    assert bc.min_give_ups(keys.numel(), n_homes) == must
    fewest = min(bc.simulate_probe(order, cap)
                 for order in _orders(keys, 50, seed=cap))
    assert fewest >= must
    # ascending order fills all reachable slots: the bound is attained
    assert bc.simulate_probe(keys.sort().values.tolist(), cap) >= must
