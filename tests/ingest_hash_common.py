"""A Python port of the hash behind device ingest's dense ids (spk_ingest.hip: mix64, hash_bytes, k_hash and
hashed_ids' four seeds), so that a test can choose a hash width (Context.ingest_set_hash_bits) at which a given set
of values collides under exactly the seeds it wants: hashed_ids re-hashes under the next seed when two different
values of one run share a key, and gives up after the fourth."""
M64 = (1 << 64) - 1
SEEDS = [0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89]
GOLDEN = 0x9E3779B97F4A7C15


def mix64(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def hash_bytes(raw, seed):
    n = len(raw)
    h = mix64(seed ^ ((n * GOLDEN) & M64))
    i = 0
    while i + 8 <= n:
        h = (mix64(h ^ int.from_bytes(raw[i:i + 8], "little")) + GOLDEN) & M64
        i += 8
    return mix64(h ^ int.from_bytes(raw[i:], "little") ^ 0x632BE59BD9B4E019)


def key_of(value, seed, bits=63):
    """k_hash's key of a non-NULL value: a str (its UTF-8 bytes) or an int (an int64 raw column's value)."""
    if isinstance(value, str):
        h = hash_bytes(value.encode("utf-8"), seed)
    else:
        h = mix64((int(value) & M64) ^ seed)
    return (h >> 1) & ((1 << bits) - 1)


def colliding_seeds(values, bits):
    """Per seed: whether two different values of `values` share a key at `bits` bits (hashed_ids then retries)."""
    distinct = set(values)
    return [len({key_of(v, s, bits) for v in distinct}) < len(distinct) for s in SEEDS]


def colliding_values(values, bits, seed=SEEDS[0]):
    """The groups of different values that share a key under `seed` at `bits` bits."""
    groups = {}
    for v in set(values):
        groups.setdefault(key_of(v, seed, bits), []).append(v)
    return [sorted(g, key=str) for g in groups.values() if len(g) > 1]


def find_bits(values, want):
    """The widest width (63 .. 1 bits) at which the seeds' collision flags match `want` (four of True / False /
    None = either), or None."""
    for bits in range(63, 0, -1):
        if all(w is None or w == c for w, c in zip(want, colliding_seeds(values, bits))):
            return bits
    return None
