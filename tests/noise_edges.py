"""Philox counters (seed 0) whose words reach the extreme uniforms of fd_u01, found once by a scan of the first 2^26 counters with
oracle.fdiff_oracle.engine_philox_words and committed as constants; tests/test_engine_randn_cpu.py re-derives every word here, and
tests/test_gpu_noise_parity.py draws fd_randn(seed = 0, offset = counter, n = 4) at each.

Lanes: 0, 1, 2, 3 = words x, y, z, w of the counter; (x, y) feed elements 0, 1 and (z, w) elements 2, 3, the first word of a pair as
u1 (the radius), the second as u2 (the angle, in revolutions)."""

EDGE_SEED = 0

# (counter, lane, word): u1 extremes
U1_ONE = (2330056, 2, 0xFFFFFF45)           # word >> 8 == 0xFFFFFF: u1 == 1.0 exactly, elements 2 and 3 are +-0
U1_BELOW_ONE = (4826271, 0, 0xFFFFFEC3)     # word >> 8 == 0xFFFFFE: u1 == 1 - 2^-23, the largest below 1 (r = 4.88e-4)
U1_SMALLEST = (14883995, 0, 0x00000093)     # word >> 8 == 0: u1 == 2^-25, the largest radius r = 5.887

# (counter, lane, word): u2 at the quadrant boundaries of the hardware sine and cosine -- word >> 8 == 0, 2^22, 2^23, 3 * 2^22, i.e.
# u2 = 2^-25, 1/4 + 2^-25, and (the + 0.5 rounded away, to even) exactly 1/2 and exactly 3/4; one counter per boundary in lane y and
# one in lane w
U2_QUADRANTS = (
    (17169035, 1, 0x000000C8), (40983361, 3, 0x000000B9),
    (7980426, 1, 0x400000CB), (9927119, 3, 0x40000091),
    (8423724, 1, 0x8000002E), (454764, 3, 0x80000001),
    (5288436, 1, 0xC0000069), (15101153, 3, 0xC0000049),
)

ALL_EDGES = (U1_ONE, U1_BELOW_ONE, U1_SMALLEST) + U2_QUADRANTS
