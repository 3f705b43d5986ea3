"""The shape thresholds at which the library switches kernels by itself -- one table for the tests that sit on them.

tests/test_gpu_switch_points.py aims its cases at these values; tests/test_switch_points_cpu.py reads every one of them back out
of the sources (the pattern beside it) and fails when a threshold moves, so the GPU cases never drift into the interior of one
path.  Entry: name -> (source file under csrc/ or include/, regular expression, the values its groups must equal, GPU test)."""

TILE_SHIFT = 10                 # finalize scan tile: 1 << TILE_SHIFT histogram slots
TILE = 1 << TILE_SHIFT
CHAIN_MAX_TILES = 512           # the chained one-launch finalize up to this many tiles (when the tile sums were not kept)
TILE_SUMS_MAX_READS = 1 << 20   # the streaming kernel keeps the tile sums below this many reads in one launch
FLIP_RATIO = 64                 # the all-boundaries-at-once walk when n_reads <= FLIP_RATIO * n_valid (nValid * 256 >= 4 * nReads)
BUCKET_MIN_READS = 1 << 18      # reads in no order: the partition path from this many reads in one batch
SCAN_BKT_MAX_BUCKETS = 4096     # scan partition tables only up to this many buckets ...
SCAN_BKT_MAX_CLASSES = 2048     # ... and this many classes
SCAN_BKT_MIN_PER = 16384        # micro-windows per scan bucket, at least (GTX_SCAN_BUCKETS default: 2000 buckets)
JOIN_SMALL_SEG = 32             # join segment sort: insertion sort per lane up to this many pairs
JOIN_LDS_SEG = 2048             # bitonic sort in LDS up to this many; runs of it + merge passes above
JOIN_SCAN_THREADS = 256         # join / entry offset scan: one block of this many lanes scans the partials ...
JOIN_SCAN_TILE = 2048           # ... of tiles of this many int64 (n + 1 offsets are scanned)
OFF_SMALL_SEG = 32              # pair offsets: one lane per query up to this many pairs, one block per query above
SIGNAL_LDS_BINS = 4096          # profile row in LDS up to this many bins

SRC = {
    "TILE_SHIFT": ("gtx_kernels.hip", r"static constexpr int kTileShift = (\d+);", (TILE_SHIFT,)),
    "CHAIN_MAX_TILES": ("gtx_kernels.hip", r"static constexpr int kChainMaxTiles = (\d+);", (CHAIN_MAX_TILES,)),
    "CHAIN_RULE": ("gtx_kernels.hip", r"if \(!tileSumsValid && chainFlags && chained && info && chainDraws && nbRun <= chainMax\)", ()),
    "HIST_LEN": ("gtx_capi.hip", r"const int64_t histLen = nv \+ nClasses;", ()),
    "TILE_SUMS_MAX_READS": ("gtx_capi.hip", r"if \(c->histLen <= lim && nReads >= \(1 << (\d+)\)\) \{ a\.partA = nullptr;", (TILE_SUMS_MAX_READS.bit_length() - 1,)),
    "HIST32_RULE": ("gtx_capi.hip", r"count_args\(c, c->ix\.hist, flags, n, 0, COUNT_ANY, d_weights == nullptr\)", ()),
    "FLIP_RULE": ("gtx_capi.hip", r"a\.flip = fl \? atoi\(fl\) : \(regions \* (\d+) >= (\d+) \* std::max<int64_t>\(nReads, 1\)\)", (4 * FLIP_RATIO, 4)),
    "BUCKET_MIN_READS": ("gtx_capi.hip", r"int64_t bucketMinReads = 1 << (\d+);", (BUCKET_MIN_READS.bit_length() - 1,)),
    "BUCKET_RULE_COUNT": ("gtx_capi.hip", r"if \(t\.nB == 0 \|\| n < c->bucketMinReads \|\| n >= \(1ll << 31\)\)", ()),
    "BUCKET_RULE_COVERAGE": ("gtx_capi.hip", r"if \(unsorted && t\.nB > 0 && n >= c->bucketMinReads && n < \(1ll << 31\)\)", ()),
    "BUCKET_RULE_SCAN": ("gtx_capi.hip", r"if \(unsorted && !a\.sortedRule && n >= c->bucketMinReads && n < \(1ll << 31\)\) \{", ()),
    "SCAN_BKT_LIMITS": ("gtx_capi.hip", r"if \(nB == 0 \|\| nB > (\d+) \|\| nClasses > (\d+) \|\|", (SCAN_BKT_MAX_BUCKETS, SCAN_BKT_MAX_CLASSES)),
    "SCAN_BKT_MIN_PER": ("gtx_capi.hip", r"long long per = std::max<long long>\((\d+), \(total \+ want - 1\) / want\);", (SCAN_BKT_MIN_PER,)),
    "JOIN_SMALL_SEG": ("gtx_join.h", r"constexpr int kJoinSmallSeg = (\d+);", (JOIN_SMALL_SEG,)),
    "JOIN_LDS_SEG": ("gtx_join.h", r"constexpr int kJoinLdsSeg = (\d+);", (JOIN_LDS_SEG,)),
    "JOIN_SCAN_TILE": ("gtx_join.hip", r"constexpr int kScanThreads = (\d+), kScanItems = (\d+), kScanTile = kScanThreads \* kScanItems;",
                       (JOIN_SCAN_THREADS, JOIN_SCAN_TILE // JOIN_SCAN_THREADS)),
    "JOIN_SCAN_N1": ("gtx_capi.hip", r"gtx::launch_join_scan\(d_off, q\.n \+ 1, ", ()),
    "OFF_SMALL_SEG": ("gtx_offset.h", r"constexpr int kOffSmallSeg = (\d+);", (OFF_SMALL_SEG,)),
    "SIGNAL_LDS_BINS": ("gtx_signal.h", r"constexpr int kSignalLdsBins = (\d+);", (SIGNAL_LDS_BINS,)),
    "SIGNAL_LDS_RULE": ("gtx_signal.hip", r"const bool lds = !a\.perRef && a\.nBins <= kSignalLdsBins;", ()),
}

# which GPU test re-aims at each entry when it moves
AIMED_BY = {
    "TILE_SHIFT": "test_finalize_routes", "CHAIN_MAX_TILES": "test_finalize_routes", "CHAIN_RULE": "test_finalize_routes",
    "HIST_LEN": "test_finalize_routes", "TILE_SUMS_MAX_READS": "test_finalize_routes", "HIST32_RULE": "test_finalize_routes",
    "FLIP_RULE": "test_flip_kernel", "BUCKET_MIN_READS": "test_unsorted_partition_path", "BUCKET_RULE_COUNT": "test_unsorted_partition_path",
    "BUCKET_RULE_COVERAGE": "test_unsorted_partition_path", "BUCKET_RULE_SCAN": "test_unsorted_partition_path",
    "SCAN_BKT_LIMITS": "test_scan_partition_tables", "SCAN_BKT_MIN_PER": "test_scan_partition_tables",
    "JOIN_SMALL_SEG": "test_join_segment_sort", "JOIN_LDS_SEG": "test_join_segment_sort", "JOIN_SCAN_TILE": "test_join_scan_partials",
    "JOIN_SCAN_N1": "test_join_scan_partials", "OFF_SMALL_SEG": "test_pair_offset_segments", "SIGNAL_LDS_BINS": "test_signal_bins_lds_limit",
    "SIGNAL_LDS_RULE": "test_signal_bins_lds_limit",
}


def tiles(n_valid, n_classes):
    """finalize scan tiles of a reference set: histLen = valid regions + classes"""
    return -(-(n_valid + n_classes) // TILE)


def join_scan_per(n_queries):
    """partials each lane of the one-block scan takes for n queries (n + 1 offsets in tiles of JOIN_SCAN_TILE)"""
    nt = -(-(n_queries + 1) // JOIN_SCAN_TILE)
    return -(-nt // JOIN_SCAN_THREADS)
