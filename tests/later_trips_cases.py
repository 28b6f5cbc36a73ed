"""What tests/test_later_trips_gpu.py and tests/test_later_trips_host.py share: the sizes at which the device loops of the frame and query
kernels turn over, worked out from the limits the library reports (render.debug_loop_limits, render.last_query_launch) and never from a
source file, and the inputs of the cases.

Every loop below runs once at the sizes of the other test files; a test here is worth something only if its size takes the loop into a later
trip, so every size comes with a function that says how many trips it makes, and the tests assert that number.

  loop                                          one trip covers                                        crossed by
  query_kernel / albedo kernels (batches)       workgroups launched x 256 rays                         workgroups x 256 + 4133 rays
  radiance_kernel / pixels_kernel (chunks)      one chunk per wave: workgroups x 4 chunks              chunks >= 2 x waves
  adaptive_scan_kernel (carry)                  1024 workgroup counts = 1 048 576 pixels               1027 x 1031 (2 trips), 1450 x 1447 (3)
  adaptive_resolve4_kernel                      1024 x 256 lanes x 4 pixels = 1 048 576 pixels         the same two shapes
  rt_denoise_frame.hip, rt_denoise_var.hip      2048 x 256 pairs of doubles = 349 525.3 pixels         601 x 587 = 352 787 pixels
  resolve_rgb8_kernel                           8192 x 256 lanes x 4 pixels = 8 388 608 pixels         2897 x 2897 = 8 392 609 pixels"""
import functools

import numpy as np

import adaptive_cases as AC

QUERY_RAYS = 4133                                  # tests/test_ray_query_gpu.py's batch
COMPACTION_SHAPES = ((1027, 1031), (1450, 1447))   # (H, W): 1035 and 2050 workgroups of the compaction; 4 k + 1 and 4 k + 2 pixels
DENOISE_SHAPE = (601, 587)                         # 352 787 pixels, 1 058 361 doubles: an odd count, so the one-double tail kernels run with first != 0
RESOLVE_SHAPE = (2897, 2897)                       # 8 392 609 pixels: one more than a multiple of 4
CHUNKS = (1, 3, 64, 100)
PATHS = 30000                                      # where the chunk cases start; raised from the launch the library reports until every wave has two chunks
IDS = dict(ids=lambda s: f"{s[1]}x{s[0]}")


def trips(n, per_trip):
    """Trips of a loop that covers per_trip items per trip over n items."""
    return -(-int(n) // int(per_trip))


def scan_trips(shape, lim):
    """adaptive_scan_kernel: the workgroup counts of the compaction, scan_threads at a time."""
    return trips(trips(shape[0] * shape[1], lim["compaction_block_px"]), lim["scan_threads"])


def adaptive_resolve_trips(shape, lim):
    """adaptive_resolve4_kernel: four pixels per lane, at most adaptive_error_max_blocks workgroups."""
    return trips((shape[0] * shape[1]) // 4, lim["adaptive_error_max_blocks"] * lim["adaptive_threads"])


def pair_trips(shape, lim, which):
    """The element-wise kernels of rt_denoise_frame.hip ("denoise_frame") and rt_denoise_var.hip ("variance"): one pair of doubles per lane."""
    return trips((shape[0] * shape[1] * 3) // 2, lim[which + "_max_blocks"] * lim[which + "_threads"])


def resolve_trips(shape, lim):
    """resolve_rgb8_kernel: resolve_px_per_lane pixels per lane, at most resolve_max_blocks workgroups."""
    return trips((shape[0] * shape[1]) // lim["resolve_px_per_lane"], lim["resolve_max_blocks"] * lim["resolve_threads"])


def paths_for_two_chunks(launch, paths):
    """From the launch the library reports for a chunked kernel: `paths` if every wave had at least two chunks, else the smallest path count
    that gives the launched waves two chunks each (a larger launch may then report more waves: the caller asks again)."""
    if launch["chunks"] >= 2 * launch["waves"]:
        return paths
    return max(paths + 1, 2 * launch["waves"] * launch["chunk"])


# ---------------------------------------------------------------- C. need maps of the compaction
def flag_state(shape, pixels):
    """A state whose selection (spread 0, tau 0.01) is exactly `pixels` (tests/test_adaptive_gpu.py's _flag_state): they hold one pass, every
    other pixel is finished beyond doubt (Q = 0: ssb clamps to 0, e2 = 0)."""
    S = np.full(shape + (3,), 16.0); Q = np.zeros(shape + (3,)); n = np.full(shape, 32, np.uint32); b = np.full(shape, 4, np.uint32)
    b.reshape(-1)[np.asarray(pixels, np.int64)] = 1
    return S, Q, n, b


def need_maps(shape, block_px=1024, scan=1024):
    """{name: ascending uint32 pixels}: empty, full, one pixel in the very last workgroup of the compaction only, one in workgroup `scan`
    (the first count of the scan's second trip) only, random at 1 % and at 50 %."""
    n_px = shape[0] * shape[1]
    rs = np.random.RandomState(31 * shape[0] + shape[1])
    last_block = (n_px - 1) // block_px
    assert last_block > scan
    return {"empty": np.zeros(0, np.uint32), "full": np.arange(n_px, dtype=np.uint32),
            "last_block": np.array([last_block * block_px + (n_px - 1 - last_block * block_px) // 2], np.uint32),
            "block_1024": np.array([scan * block_px + 517], np.uint32),
            "random_1pc": np.flatnonzero(rs.rand(n_px) < 0.01).astype(np.uint32),
            "random_50pc": np.flatnonzero(rs.rand(n_px) < 0.5).astype(np.uint32)}


@functools.lru_cache(maxsize=None)
def big_state(shape):
    """adaptive_cases.state at a large shape (S, Q, n, b), read-only, built once."""
    return AC.state(shape)
