"""Scratch buffers of the PLAN engines replaced IN FLIGHT (``csrc/plan_gpu.hip``: the device scratch of a set, the shared
pinned staging blocks, the per-set pinned tables).

The engines take their scratch sets in rotation -- contig ``i`` of a pass meets set ``i mod 32`` -- and a buffer that is too small
is freed and allocated again, behind a wait for everything that may still use the old block.  A pass of at most 32 contigs
never meets that path with work queued; these genomes have 40 contigs and NO warm-up step, so the step whose bytes are read
back is the step in which the buffers are replaced:

* ``late``: 32 contigs of length ``a``, then 8 of ``3a`` -- sets 0-7 are outgrown (a block holds 1.25 x what was asked + 4 KB, so
  ``3a`` exceeds every capacity) while the emission of earlier contigs may still be queued;
* ``alternating``: ``a, 3a, a, 3a, ...`` -- an even set starts small and meets a ``3a`` contig on its second use, an odd set
  keeps a block larger than its second user needs.

``a`` per workload, the smallest round length at which the engine still takes all 40 contigs (the engine counter is asserted):
c2 450 000 (the SNP sampler wants k >= 4096 draws per range: 409 600 bases of ``-sn 0.01``), c3 600 000 (likewise for the SV
mix, whose rates add up to 0.008: 512 000 bases), c4 300 000, c4sv 600 000 (the host-chain engine wants 1 024 candidates per
contig; the gene-blocking file leaves 864 of them on its sparsest 300 kb contig, 1 254 on 600 kb).

Everything ``_bench_order_vs_oracle`` checks holds: Fasta body and VCF text of every contig and both final stream positions
against the CPU oracle."""
from __future__ import annotations

import pytest

from test_gpu_bench_order import _bench_order_vs_oracle

pytestmark = pytest.mark.gpu

N_CONTIGS = 40

WORKLOADS = [("c2", "contigs_snp", 450_000), ("c3", "contigs_svmix", 600_000), ("c4", "contigs_hostcut", 300_000),
             ("c4sv", "contigs_hostchain", 600_000)]


def _lengths(pattern, a):
    if pattern == "late":
        return [a] * 32 + [3 * a] * 8
    return [a, 3 * a] * (N_CONTIGS // 2)


@pytest.mark.parametrize("pattern", ["late", "alternating"])
@pytest.mark.parametrize("workload,counter,a", WORKLOADS)
def test_scratch_replaced_in_flight_vs_oracle(workload, counter, a, pattern):
    lengths = _lengths(pattern, a)
    assert len(lengths) == N_CONTIGS
    st = _bench_order_vs_oracle(workload, lengths, warmup=False)
    assert st[counter] == N_CONTIGS, {k: v for k, v in st.items() if k.startswith("contigs_") and v}
