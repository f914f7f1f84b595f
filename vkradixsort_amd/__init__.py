"""vkradixsort_amd -- MI355X-native multi-block LSD radix sort behind VkRadixSort's MultiRadixSort host API.

csrc/    hand-written gfx950 HIP kernels + the C ABI (include/vkradixsort_amd*.h)
host/    C++ mirror of the reference's host classes (engine::GPUContext, Buffer, MultiRadixSortPass, ...)
engine   the same interface for Python callers (tests, bench.py), a thin ctypes layer over the C ABI
segmented  many independent segments sorted in one call (sort_segments over Buffers, sort_rows for 2-D torch tensors)
topk       the k smallest / largest keys of every segment by radix select (topk_segments over Buffers, topk for torch tensors); the
           torch.topk drop-in: nine dtypes, any dim and strides, torch's order, the elements' own bits (torch_topk)
selection  torch.kthvalue / torch.median / torch.nanmedian drop-ins by a one-rank radix select: nine dtypes, any dim (select_segments over
           Buffers; kthvalue, median, nanmedian for torch tensors)
quantile   torch.quantile / torch.nanquantile drop-ins by a multi-rank radix select: up to 16 order statistics per row carried through one
           sequence of reads, values only (quantile_segments over Buffers; quantile, nanquantile for torch tensors)
sort       torch.sort / torch.argsort drop-ins: any dim, descending, nine dtypes, torch's order bit for bit (sort, sort_values, argsort)
mode       torch.mode drop-in: the most frequent value of every row and the last index where it sits, by a bare-key sort of the ranks and
           the mode form of vrs_sort_restore -- the longest run of every sorted row, no position payload through the sort (mode)
search     torch.searchsorted / torch.bucketize drop-ins over sorted sequences: nine dtypes, N-D, sorter (searchsorted, bucketize);
           torch.isin by a sort of the test set and the search's membership form, a byte per element (isin)
binning    torch.bincount / torch.histc / torch.histogram drop-ins: counters in LDS or global memory, integer counts converted once
           (bincount, histc, histogram)
reduce     torch.segment_reduce / index_add / index_reduce / scatter_reduce drop-ins with reproducible sums: a segmented reduction over
           rows in a fixed order (segment_reduce, index_add, index_reduce, scatter_reduce)
scan       torch.cumsum / cumprod / cummax / cummin drop-ins: an inclusive prefix scan along any dim in a fixed order, the same bits on
           every run (cumsum, cumprod, cummax, cummin)
compact    torch.nonzero / argwhere / where(condition) / count_nonzero / masked_select / masked_scatter drop-ins: ordered stream compaction
           in three phases that wait nowhere -- count, carries, emit (nonzero, argwhere, where, count_nonzero, masked_select,
           masked_scatter); and x[mask] / index_put with a mask over the leading dims, every flag a whole row (mask_index,
           mask_index_put)
repeat     torch.repeat_interleave drop-in: run-length decode, the undo of unique_consecutive(return_counts=True) -- cumsum, then the
           identity form of the sorted search (a merge: boundaries read once, indices written once), then index_select
           (repeat_interleave)
unique     run-length encoding and unique by sort + encode (run_length_encode / unique_keys over Buffers, unique / unique_consecutive
           for torch tensors); with dim=d (columns=C over Buffers) the distinct rows: LSD rounds of pack + stable pair sort over groups
           of columns, then the encode with a row head rule
"""
from .binning import bincount, bincount_stats, histc, histogram  # noqa: F401
from .capi import PushConstants, VrsError, load_library  # noqa: F401
from .compact import (argwhere, compact_stats, count_nonzero, mask_index, mask_index_put, masked_scatter,  # noqa: F401
                      masked_select, nonzero, where)
from .engine import (Buffer, ComputePass, Extent3D, GPUContext, MultiRadixSort, MultiRadixSortPass,  # noqa: F401
                     SingleRadixSort, SingleRadixSortPass, generateRandomNumbers)
from .mode import mode  # noqa: F401
from .quantile import nanquantile, quantile, quantile_scratch_bytes, quantile_segments, quantile_stats  # noqa: F401
from .reduce import index_add, index_reduce, reduce_stats, scatter_reduce, segment_reduce  # noqa: F401
from .repeat import repeat_interleave  # noqa: F401
from .scan import cummax, cummin, cumprod, cumsum, scan_stats  # noqa: F401
from .search import bucketize, isin, search_stats, searchsorted  # noqa: F401
from .segmented import segmented_stats, sort_rows, sort_segments  # noqa: F401
from .selection import kthvalue, median, nanmedian, select_scratch_bytes, select_segments, select_stats  # noqa: F401
from .sort import argsort, sort, sort_values  # noqa: F401
from .topk import topk, topk_segments, topk_stats, torch_topk  # noqa: F401
from .unique import run_length_encode, unique, unique_consecutive, unique_keys  # noqa: F401

__version__ = "0.1.0"
