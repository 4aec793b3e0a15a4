"""Command line of ``mutation-simulator`` -- flag-for-flag the reference's ``args`` and ``rmt``
sub-commands (reference argument_parser.py:31-240) plus a few additions of ours that never change
a default: ``--seed``, ``--device``, ``--gpus``, ``--rng``, ``--bgzip``, ``--chain``, ``--ploidy``, ``--het``, ``--bench-json``, ``--spectrum`` / ``--signature``
(options of ``args``: SNPs drawn per trinucleotide context, ``spectrum.py``; ``spectrum_refusal`` words what such a run does not cover), and the ``vcf`` sub-command
(``vcf_replay.py``: the mutated Fasta again from the reference and a run's VCF; it writes ``<outbase>_ms.fa`` and, with
``--chain``, ``<outbase>_ms.chain``; with ``--consensus [--sample NAME] [--haplotype N]`` the VCF may come from anywhere), and the ``profile`` sub-command (``profile.py``:
the SBS-96 spectrum of a VCF's SNPs against the reference, counted on the GPU; it writes ``<outbase>_ms.sbs96.tsv``, a file
``--spectrum`` reads; ``profile_refusal`` words what it does not cover), and the ``compare`` sub-command (``compare.py``: a calls
VCF scored against a truth VCF on the GPU, indels matched up to their placement inside a repeat; it writes
``<outbase>_ms.compare.tsv`` and, with ``--list``, ``<outbase>_ms.compare.records.tsv``; ``--diploid`` joins both haplotypes of each
side and scores genotypes by dosage -- a ``GT`` column, ``GT`` lines in the records file; it is a usage error together with
``--haplotype`` or ``--truth-haplotype``; ``--blocks [--block-gap N]`` rescues unmatched records whose block of neighbours writes
the same bases on both sides -- ``BLK`` columns and lines; a usage error together with ``--diploid``, as is ``--block-gap`` without
``--blocks``; ``--diploid --phased`` also compares the phasing and writes ``<outbase>_ms.compare.phase.tsv`` (``outcompare_phase``),
a usage error without ``--diploid`` or with ``--blocks``; ``--regions FILE`` scores only the records whose anchor -- an indel's
leftmost placement, else the position -- lies inside the BED's intervals, and the repeatable ``--stratify NAME=FILE`` adds a
genome-wide table per BED, inside ``--regions`` where both are given; NAME is non-empty, without tab, blank, ``=`` or ``#``, and
distinct; both are usage errors together with ``--phased``, whose phase table would silently stay genome-wide, and go with
``--diploid``, ``--blocks``, ``--exact``, ``--per-contig`` and ``--list``; ``compare_refusal`` words what it does not cover), and the
``reads`` sub-command (``reads.py``: FASTQ reads drawn from the genome on the GPU, ``(-n N | --coverage X) [-l LEN] [--paired
--frag-mean M --frag-sd SD] [--error-rate A[:B]] [--prefix P]``; it writes ``<outbase>_ms.fq`` (``args.outfastq``) or, with
``--paired``, ``<outbase>_ms_1.fq`` and ``<outbase>_ms_2.fq`` (``outfastq_1`` / ``outfastq_2``), ``.gz`` appended under ``--bgzip``;
``--frag-*`` without ``--paired``, ``--paired`` without both, SD > 511 and M + 4 SD < LEN are usage errors; ``reads_refusal`` words
what it does not cover).

``--ploidy 2 [--het F]`` (``args`` / ``rmt``) writes two haplotype Fastas, ``<outbase>_ms_h1<suffix>`` and ``<outbase>_ms_h2<suffix>``
(``args.outfasta_h1`` / ``outfasta_h2``; ``<outbase>_ms<suffix>`` is not written), one phased ``<outbase>_ms.vcf`` and, with ``--chain``,
``<outbase>_ms_h1.chain`` / ``_h2.chain`` (``outchain_h1`` / ``outchain_h2``).  ``ploidy_refusal`` words what a diploid run does not cover.

The ``it`` sub-command (inter-chromosomal translocations, reference it_mutator.py: a second pass over
the Fasta) runs through ``ITMutator`` / ``BedpeWriter``.  ``--rng fast`` applies to the mutation pass
(``args`` / ``rmt``) only: the IT pass always draws from CPython's generator.
"""
from __future__ import annotations

from argparse import ArgumentParser, Namespace
from pathlib import Path

from ._version import __version__
from .defaults import Defaults as D
from .fasta_io import is_gzip


def add_outfile_names(args: Namespace) -> Namespace:
    """``<outbase>_ms<infile suffix>`` / ``<outbase>_ms.vcf`` (reference argument_parser.py:14-28), and ``<outbase>_ms.chain``
    for ``--chain`` (plain text also under ``--bgzip``).

    ``-o`` may be a basename or a directory-like path with an empty stem (".", "dir/.."): then the
    input's stem is used inside that directory.

    For an input that IS gzip-compressed (by content: it exists and starts with the gzip magic) a trailing ``.gz`` /
    ``.bgz`` of its name is dropped before the names are derived: ``genome.fa.gz`` gives ``genome_ms.fa`` +
    ``genome_ms.vcf``.  Every other input -- a text Fasta whatever its name -- keeps the reference's names.
    """
    infile = args.infile
    if infile.suffix.lower() in (".gz", ".bgz") and infile.stem and is_gzip(infile):
        infile = infile.with_suffix("")
    try:
        args.outbase = args.outbase.with_stem(args.outbase.stem + "_ms")
    except ValueError:
        args.outbase = args.outbase / (infile.stem + "_ms")
    args.outfasta = args.outbase.with_suffix(infile.suffix)
    args.outfastait = args.outfasta.with_stem(args.outfasta.stem + "_it")
    args.outvcf = args.outfasta.with_suffix(".vcf")
    args.outbedpe = args.outfastait.with_suffix(".bedpe")
    args.outchain = args.outfasta.with_suffix(".chain")
    if getattr(args, "mode", None) == "profile":  # (only there: the other modes' namespaces stay as they were)
        args.outprofile = args.outfasta.with_suffix(".sbs96.tsv")
    if getattr(args, "mode", None) == "compare":
        args.outcompare = args.outfasta.with_suffix(".compare.tsv")
        args.outcompare_records = args.outfasta.with_suffix(".compare.records.tsv")
        args.outcompare_phase = args.outfasta.with_suffix(".compare.phase.tsv")
    if getattr(args, "mode", None) == "reads":
        gz = ".gz" if getattr(args, "bgzip", False) else ""
        stem = args.outfasta.stem
        args.outfastq = args.outfasta.with_name(f"{stem}.fq{gz}")
        args.outfastq_1 = args.outfasta.with_name(f"{stem}_1.fq{gz}")
        args.outfastq_2 = args.outfasta.with_name(f"{stem}_2.fq{gz}")
    if getattr(args, "ploidy", 1) == 2:           # a diploid run: a Fasta (and a chain) per haplotype, ONE phased VCF
        for h in ("h1", "h2"):
            fa = args.outfasta.with_stem(f"{args.outfasta.stem}_{h}")
            setattr(args, f"outfasta_{h}", fa)
            setattr(args, f"outchain_{h}", fa.with_suffix(".chain"))
    if getattr(args, "bgzip", False):             # BGZF-compressed mutation-pass outputs: <name>.gz
        args.outfasta = args.outfasta.with_name(args.outfasta.name + ".gz")
        args.outvcf = args.outvcf.with_name(args.outvcf.name + ".gz")
    return args


# (short, long, kind, default, help) for one mutation type: rate / min / max / block
def _type_options(short: str, long: str, label: str, plural: str, minlen, maxlen, after: str):
    opts = [(f"-{short}", f"--{long}", float, D.RATE, f"{label} rate. Default = {D.RATE}")]
    if minlen is not None:
        opts.append((f"-{short}min", f"--{long}minlength", int, minlen,
                     f"Minimum length of {plural}. Default = {minlen}"))
        opts.append((f"-{short}max", f"--{long}maxlength", int, maxlen,
                     f"Maximum length of {plural}. Default = {maxlen}"))
    opts.append((f"-{short}b", f"--{long}block", int, D.BLOCK,
                 f"Amount of bases blocked after {after}. Default = {D.BLOCK}"))
    return opts


def build_parser() -> ArgumentParser:
    parser = ArgumentParser(
        prog="mutation-simulator",
        description="See https://github.com/mkpython3/Mutation-Simulator for more information "
                    "about this program.")
    parser.add_argument("infile", type=Path, help="Path of the reference Fasta file")
    parser.add_argument("-o", "--output", type=Path, default=D.OUTBASE, dest="outbase",
                        help="Path/Basename for the output files (without file extension)")
    for flag, long, default, text in (
            ("-w", "--ignore-warnings", D.IGNORE_WARNINGS, "Silences warnings"),
            ("-c", "--no-color", D.NO_COLOR, "Always disable color"),
            ("-p", "--no-progress", D.NO_PROGRESS, "Disable progressbars"),
            ("-q", "--quiet", D.QUIET, "Disable all output except errors")):
        parser.add_argument(flag, long, action="store_true", default=default, help=text)
    parser.add_argument("-v", "--version", action="version",
                        version=f"Mutation-Simulator {__version__}")
    # additions of this build (defaults keep the reference's behaviour)
    parser.add_argument("--seed", type=int, default=None,
                        help="Seed both random streams (random.seed(S); numpy.random.seed(S)) "
                             "for reproducible output")
    parser.add_argument("--device", type=int, default=0, help="GPU ordinal to run on")
    parser.add_argument("--gpus", type=int, default=1,
                        help="Shard the contigs over this many GPUs of the node (one worker process per GPU; output is "
                             "byte-identical to a 1-GPU run). Default = 1")
    parser.add_argument("--rng", choices=["compat", "fast"], default="compat",
                        help="compat (default): the reference's two MT19937 streams, output bit-identical to the reference "
                             "under the same seeds. fast: a counter-based generator (Philox) -- same distributions, NOT the "
                             "reference's numbers; no sequential chain in the draw; SNP-only settings")
    parser.add_argument("--bgzip", action="store_true", default=False,
                        help="Write the mutated Fasta and the VCF BGZF-compressed (<name>.gz, compressed on the GPU); "
                             "they decompress to exactly the files written without it. Not with it / --gpus N > 1")
    parser.add_argument("--chain", action="store_true", default=False,
                        help="Also write <outbase>_ms.chain: a UCSC liftover chain per contig from the reference's coordinates "
                             "(target) to the mutated genome's (query), rendered on the GPU from the mutation table. Plain text "
                             "also with --bgzip. The run goes contig by contig (an assembly of thousands of small scaffolds "
                             "loses the speed of the batched pass; the output bytes are the same). Not with it / it lines in "
                             "the RMT / --gpus N > 1")
    parser.add_argument("--ploidy", type=int, choices=[1, 2], default=1,
                        help="2: a diploid run -- the mutation pass of --ploidy 1, then every mutation is given a genotype and "
                             "the run writes two haplotype Fastas (<outbase>_ms_h1, <outbase>_ms_h2 instead of <outbase>_ms), one "
                             "VCF with phased genotypes (1|0, 0|1, 1|1) and, with --chain, a chain file per haplotype. The run "
                             "goes contig by contig. Not with it / it lines in the RMT / vcf / --gpus N > 1 / --bgzip. Default = 1")
    parser.add_argument("--het", type=float, default=None, metavar="F",
                        help="With --ploidy 2: the fraction of heterozygous mutations, in [0, 1]; a heterozygous mutation is on "
                             "haplotype 1 or 2 with equal chance, every other one on both. Default = 0.5")
    parser.add_argument("--bench-json", type=Path, default=None,
                        help="Write per-stage timings of the mutation pass to this JSON file")

    sub = parser.add_subparsers(
        dest="mode",
        help="Generate mutations or interchromosomal translocations via RMT or arguments")
    sub.required = True

    p_args = sub.add_parser("args", help="Use commandline arguments for mutations instead of RMT")
    table = _type_options("sn", "snp", "SNP", "", None, None, "SNP")
    table.insert(2, ("-titv", "--transitionstransversions", float, D.TITV,
                     f"Ratio of transitions:transversions likelihood. Default = {D.TITV}"))
    table += _type_options("in", "insert", "Insert", "inserts", D.MINLEN, D.MAXLEN, "insert")
    table += _type_options("de", "deletion", "Deletion", "deletions", D.MINLEN, D.MAXLEN,
                           "deletion")
    table += _type_options("iv", "inversion", "Inversion", "inversion", D.IV_MINLEN, D.IV_MAXLEN,
                           "inversion")
    table += _type_options("du", "duplication", "Duplication", "duplications", D.MINLEN,
                           D.MAXLEN, "duplication")
    table += _type_options("tl", "translocation", "Translocation", "translocations", D.MINLEN,
                           D.MAXLEN, "translocations")
    for short, long, kind, default, text in table:
        p_args.add_argument(short, long, type=kind, default=default, help=text)
    for short, long, default, what in (("-a", "--assembly", D.ASSEMBLY_NAME, "Assembly"),
                                       ("-s", "--species", D.SPECIES_NAME, "Species"),
                                       ("-n", "--sample", D.SAMPLE_NAME, "Sample")):
        p_args.add_argument(short, long, default=default,
                            help=f"{what} name for the VCF file. Default = '{default}'")

    p_args.add_argument("--spectrum", type=Path, default=None, metavar="FILE",
                        help="Draw the SNPs per trinucleotide context from a 96-channel mutational spectrum (rows N[X>Y]N with X in "
                             "C, T -- COSMIC's SBS tables as published): every site mutates independently, -sn is the expected "
                             "fraction of a contig's sites, the file decides which. -snb and -titv do not apply. Needs --rng fast; "
                             "SNPs only; not with --gpus N > 1")
    p_args.add_argument("--signature", default=None, metavar="NAME",
                        help="With --spectrum: the column of the file's header to use. Default = the first value column")

    p_it = sub.add_parser("it", help="Generate interchromosomal translocations via the command line")
    p_it.add_argument("interchromosomalrate", type=float,
                      help="Rate of interchromosomal translocations")

    p_rmt = sub.add_parser("rmt", help="Use random mutation table instead of arguments")
    p_rmt.add_argument("rmtfile", type=Path, help="Path to the RMT file")

    p_vcf = sub.add_parser("vcf", help="Rebuild the mutated Fasta from the reference Fasta and the VCF of a run")
    p_vcf.add_argument("vcffile", type=Path, help="Path to the VCF file (text or BGZF-compressed)")
    p_vcf.add_argument("--consensus", action="store_true", default=False,
                       help="Take any VCF, not only one this program wrote: apply one haplotype of one sample, as "
                            "bcftools consensus -s SAMPLE -H N does")
    p_vcf.add_argument("--sample", default=None, metavar="NAME",
                       help="With --consensus: the sample column to follow. Default = the first one")
    p_vcf.add_argument("--haplotype", type=int, default=None, metavar="N",
                       help="With --consensus: which allele of the genotype to apply, counted from 1. Default = 1")

    p_prof = sub.add_parser("profile", help="Count the SBS-96 spectrum of a VCF's SNPs against the reference Fasta: a file "
                                            "args --spectrum reads")
    p_prof.add_argument("vcffile", type=Path, help="Path to the VCF file (text or BGZF-compressed)")
    p_prof.add_argument("--consensus", action="store_true", default=False,
                        help="Take any VCF, not only one this program wrote: count one haplotype of one sample, the "
                             "records vcf --consensus would apply")
    p_prof.add_argument("--sample", default=None, metavar="NAME",
                        help="With --consensus: the sample column to follow. Default = the first one")
    p_prof.add_argument("--haplotype", type=int, default=None, metavar="N",
                        help="With --consensus: which allele of the genotype to count, counted from 1. Default = 1")
    p_prof.add_argument("--per-contig", action="store_true", default=False, dest="per_contig",
                        help="Add one column per contig, named by the contig, behind the genome-wide one")
    p_prof.add_argument("--name", default="profile", metavar="NAME",
                        help="Name of the genome-wide column (what --signature picks). Default = 'profile'")

    p_cmp = sub.add_parser("compare", help="Score a calls VCF against a truth VCF on the reference Fasta: recall and precision "
                                           "per variant type and length, indels matched wherever a repeat lets them stand")
    p_cmp.add_argument("truthfile", type=Path, help="Path to the truth VCF file (text or BGZF-compressed)")
    p_cmp.add_argument("callsfile", type=Path, help="Path to the calls VCF file (text or BGZF-compressed)")
    p_cmp.add_argument("--truth-sample", default=None, metavar="NAME", dest="truth_sample",
                       help="The sample column of the truth VCF to follow. Default = the first one")
    p_cmp.add_argument("--truth-haplotype", type=int, default=None, metavar="N", dest="truth_haplotype",
                       help="Which allele of the truth genotype to score against, counted from 1. Default = 1")
    p_cmp.add_argument("--sample", default=None, metavar="NAME",
                       help="The sample column of the calls VCF to follow. Default = the first one")
    p_cmp.add_argument("--haplotype", type=int, default=None, metavar="N",
                       help="Which allele of the calls genotype to score, counted from 1. Default = 1")
    p_cmp.add_argument("--diploid", action="store_true", default=False,
                       help="Score genotypes against a diploid truth: both haplotypes of each side are joined into distinct "
                            "variants with a dosage (0/1 or 1/1, phase ignored; a haploid 1 counts as 1/1); a variant found with "
                            "the wrong dosage is reported as GT. Cannot be combined with --truth-haplotype or --haplotype")
    p_cmp.add_argument("--phased", action="store_true", default=False,
                       help="With --diploid: also compare the phasing of the matched heterozygous variants against the truth's "
                            "(GT written with |, PS naming the phase set) and write <outbase>_ms.compare.phase.tsv: switch errors, "
                            "switches and flips, blockwise Hamming distance. Cannot be combined with --blocks")
    p_cmp.add_argument("--exact", action="store_true", default=False,
                       help="Compare positions literally: an indel placed elsewhere in its repeat counts as missed and as extra")
    p_cmp.add_argument("--blocks", action="store_true", default=False,
                       help="Rescue unmatched records block by block: neighbouring records of both files are replayed onto the "
                            "reference, and where the truth's and the calls' records of a block write the same bases (an MNP "
                            "against two SNPs, a duplication against the insertion it is) they count as matched (BLK columns). "
                            "Cannot be combined with --diploid")
    p_cmp.add_argument("--block-gap", type=int, default=None, metavar="N", dest="block_gap",
                       help="With --blocks: a record joins the block in front of it when it stands at most N bases behind it "
                            "(0 to 4096). Default = 50")
    p_cmp.add_argument("--regions", type=Path, default=None, metavar="FILE",
                       help="Score only the records inside the intervals of this BED file (text, .gz or .bgz), the truth set's "
                            "confident regions: a record counts by its anchor, an indel's leftmost placement, so both records of a "
                            "matched pair fall on the same side of every edge. Cannot be combined with --phased")
    p_cmp.add_argument("--stratify", action="append", default=None, metavar="NAME=FILE",
                       help="Also write a genome-wide table of the records inside this BED file (and inside --regions), headed "
                            "'# stratum NAME'. May be given several times with distinct names. Cannot be combined with --phased")
    p_cmp.add_argument("--per-contig", action="store_true", default=False, dest="per_contig",
                       help="Repeat the table per contig behind the genome-wide one")
    p_cmp.add_argument("--list", action="store_true", default=False, dest="list_records",
                       help="Also write <outbase>_ms.compare.records.tsv: one line per unmatched record")

    p_reads = sub.add_parser("reads", help="Draw FASTQ reads from the genome on the GPU: single-end, or pairs from fragments of "
                                           "normally distributed length, with a per-cycle substitution error ramp")
    p_reads.add_argument("-n", "--reads", type=int, default=None, dest="n_reads", metavar="N",
                         help="Number of reads (pairs with --paired), 1 to 2^32 - 1. One of -n and --coverage is needed")
    p_reads.add_argument("--coverage", type=float, default=None, metavar="X",
                         help="Number of reads from the coverage: N = floor(X * G / (LEN * mates)), G the bases of the contigs "
                              "long enough to hold the longest fragment")
    p_reads.add_argument("-l", "--length", type=int, default=150, metavar="LEN", help="Read length, 1 to 512. Default = 150")
    p_reads.add_argument("--paired", action="store_true", default=False,
                         help="Draw pairs: mate 1 from the fragment's start, mate 2 from its end off the other strand. Needs "
                              "--frag-mean and --frag-sd; writes <outbase>_ms_1.fq and <outbase>_ms_2.fq")
    p_reads.add_argument("--frag-mean", type=int, default=None, dest="frag_mean", metavar="M",
                         help="With --paired: mean fragment length")
    p_reads.add_argument("--frag-sd", type=int, default=None, dest="frag_sd", metavar="SD",
                         help="With --paired: standard deviation of the fragment length, 0 to 511; lengths beyond M +- 4 SD (and "
                              "below LEN) are not drawn")
    p_reads.add_argument("--error-rate", default="0.001:0.01", dest="error_rate", metavar="A[:B]",
                         help="Substitution probability per cycle, linear from A at the first cycle to B at the last; a single "
                              "value is a flat rate. Default = 0.001:0.01")
    p_reads.add_argument("--prefix", default="r", metavar="P",
                         help="Prefix of the read names: letters, digits and ._- only, at most 32 bytes. Default = 'r'")
    return parser


def reads_refusal(args: Namespace):
    """What the ``reads`` mode does not cover, as the message to refuse it with; None: the run can go ahead (or is no reads
    run).  ``--rng`` has no effect: no generator of the mutation engines is touched."""
    if args.mode != "reads":
        return None
    if getattr(args, "ploidy", 1) == 2:
        return ("--ploidy 2 does not apply to the reads mode (it samples one genome: run reads on the _h1 and the _h2 Fasta "
                "with two prefixes)")
    if getattr(args, "chain", False):
        return "--chain does not apply to the reads mode (nothing is applied: there is no mutated genome to lift over to)"
    if (args.gpus or 1) > 1:
        return "the reads mode needs a single-GPU run (--gpus 1)"
    return None


def compare_refusal(args: Namespace):
    """What the ``compare`` mode does not cover, as the message to refuse it with; None: the run can go ahead (or is no
    compare).  ``--seed`` and ``--rng`` have no effect, as in ``vcf``: nothing is drawn."""
    if args.mode != "compare":
        return None
    if getattr(args, "ploidy", 1) == 2:
        return ("--ploidy 2 does not apply to the compare mode (it scores one haplotype against one: "
                "compare --truth-haplotype N --haplotype N)")
    if getattr(args, "chain", False):
        return "--chain does not apply to the compare mode (nothing is applied: there is no mutated genome to lift over to)"
    if getattr(args, "bgzip", False):
        return "--bgzip does not apply to the compare mode (it writes small text tables)"
    if (args.gpus or 1) > 1:
        return "the compare mode needs a single-GPU run (--gpus 1)"
    return None


def profile_refusal(args: Namespace):
    """What the ``profile`` mode does not cover, as the message to refuse it with; None: the run can go ahead (or is no
    profile).  ``--seed`` and ``--rng`` have no effect, as in ``vcf``: nothing is drawn."""
    if args.mode != "profile":
        return None
    if getattr(args, "ploidy", 1) == 2:
        return "--ploidy 2 does not apply to the profile mode (it counts one haplotype: profile --consensus --haplotype N)"
    if getattr(args, "chain", False):
        return "--chain does not apply to the profile mode (nothing is applied: there is no mutated genome to lift over to)"
    if getattr(args, "bgzip", False):
        return "--bgzip does not apply to the profile mode (it writes one small text table)"
    if (args.gpus or 1) > 1:
        return "the profile mode needs a single-GPU run (--gpus 1)"
    return None


def ploidy_refusal(args: Namespace, has_it: bool = False):
    """What a ``--ploidy 2`` run does not cover, as the message to refuse it with; None: the run can go ahead.  ``has_it``: the
    settings hold interchromosomal translocations (``it`` lines of an RMT -- known once the RMT is read)."""
    if getattr(args, "ploidy", 1) != 2:
        return None
    if args.mode == "it":
        return "--ploidy 2 does not apply to the interchromosomal pass (it)"
    if has_it:
        return "--ploidy 2 does not apply to the interchromosomal pass (it lines in the RMT)"
    if args.mode == "vcf":
        return "--ploidy 2 does not apply to the vcf mode (it replays one haplotype: vcf --consensus --haplotype N)"
    if (args.gpus or 1) > 1:
        return "--ploidy 2 needs a single-GPU run (--gpus 1)"
    if getattr(args, "bgzip", False):
        return ("--ploidy 2 does not write BGZF yet (--bgzip): a second Fasta stream needs a third BGZF output channel, "
                "which is a follow-up; compress the three files afterwards (bgzip)")
    return None


def spectrum_refusal(args: Namespace):
    """What a ``--spectrum`` run does not cover, as the message to refuse it with; None: the run can go ahead (or has no
    spectrum)."""
    if getattr(args, "spectrum", None) is None:
        return None
    if args.mode != "args":
        return f"--spectrum does not apply to the {args.mode} mode (it belongs to args: -sn RATE --spectrum FILE)"
    if getattr(args, "rng", "compat") != "fast":
        return ("--spectrum needs --rng fast: its SNPs are drawn per site from a counter-based generator and are not the "
                "reference's numbers under any seed (--rng compat promises those)")
    rates = {"-in": args.insert, "-de": args.deletion, "-iv": args.inversion, "-du": args.duplication, "-tl": args.translocation}
    others = [flag for flag, rate in rates.items() if rate]
    if others:
        return (f"--spectrum draws SNPs only ({', '.join(others)} given): structural variants beside a spectrum are a follow-up; "
                "run them as a second pass")
    if not args.snp:
        return "--spectrum needs an SNP rate (-sn RATE): the expected fraction of a contig's sites that mutate"
    if (args.gpus or 1) > 1:
        return "--spectrum needs a single-GPU run (--gpus 1)"
    return None


def get_args(argv=None) -> Namespace:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.het is not None and args.ploidy != 2:
        parser.error("--het needs --ploidy 2")
    if args.het is not None and not 0.0 <= args.het <= 1.0:      # (NaN fails both comparisons)
        parser.error("--het is a fraction in [0, 1]")
    if args.ploidy == 2 and args.het is None:
        args.het = 0.5
    if getattr(args, "signature", None) is not None and args.spectrum is None:
        parser.error("--signature needs --spectrum")
    if args.mode == "vcf" and args.ploidy != 2:        # (the namespace of a replay stays as it was; --ploidy 2 is refused later)
        del args.ploidy, args.het
    if args.mode == "vcf":
        if not args.consensus and (args.sample is not None or args.haplotype is not None):
            parser.error("--sample and --haplotype need --consensus")
        if args.haplotype is not None and args.haplotype < 1:
            parser.error("--haplotype counts from 1")
        if not args.consensus:                         # (the namespace of a plain replay stays as it was)
            del args.consensus, args.sample, args.haplotype
    if args.mode == "profile":
        if not args.consensus and (args.sample is not None or args.haplotype is not None):
            parser.error("--sample and --haplotype need --consensus")
        if args.haplotype is not None and args.haplotype < 1:
            parser.error("--haplotype counts from 1")
    if args.mode == "compare":
        if any(h is not None and h < 1 for h in (args.haplotype, args.truth_haplotype)):
            parser.error("--haplotype and --truth-haplotype count from 1")
        if args.diploid and (args.haplotype is not None or args.truth_haplotype is not None):
            parser.error("--diploid scores both haplotypes of each side: --haplotype and --truth-haplotype do not apply")
        if args.block_gap is not None and not args.blocks:
            parser.error("--block-gap needs --blocks")
        if args.blocks and args.diploid:
            parser.error("--blocks compares one haplotype against one: it cannot be combined with --diploid")
        if args.phased and args.blocks:
            parser.error("--phased compares the phasing of a diploid comparison: it cannot be combined with --blocks")
        if args.phased and not args.diploid:
            parser.error("--phased needs --diploid")
        if args.block_gap is not None and not 0 <= args.block_gap <= 4096:
            parser.error("--block-gap must lie in 0..4096")
        if args.phased and (args.regions is not None or args.stratify):
            parser.error("--regions and --stratify restrict the counts table only: the phase table of --phased would silently "
                         "stay genome-wide, so they cannot be combined with it")
        strata = []
        for item in args.stratify or ():
            name, sep, path = item.partition("=")
            if not sep or not name or not path or any(ch in name for ch in "\t #"):
                parser.error(f"--stratify takes NAME=FILE, NAME non-empty and without tab, blank, = or #: {item!r}")
            if name in (n for n, _ in strata):
                parser.error(f"--stratify names must be distinct: {name!r} is given twice")
            strata.append((name, Path(path)))
        args.stratify = strata
    if args.mode == "reads":
        from .reads import MAX_LEN, MAX_SD, parse_error_rate, prefix_refusal, ReadsError
        if (args.n_reads is None) == (args.coverage is None):
            parser.error("reads needs exactly one of -n N and --coverage X")
        if args.n_reads is not None and not 1 <= args.n_reads < 2**32:
            parser.error("-n must lie in 1..2^32 - 1")
        if args.coverage is not None and not 0.0 < args.coverage < float("inf"):
            parser.error("--coverage must be a positive number")
        if not 1 <= args.length <= MAX_LEN:
            parser.error(f"-l must lie in 1..{MAX_LEN}")
        if not args.paired and (args.frag_mean is not None or args.frag_sd is not None):
            parser.error("--frag-mean and --frag-sd need --paired")
        if args.paired:
            if args.frag_mean is None or args.frag_sd is None:
                parser.error("--paired needs --frag-mean and --frag-sd")
            if not 0 <= args.frag_sd <= MAX_SD:
                parser.error(f"--frag-sd must lie in 0..{MAX_SD}")
            if args.frag_mean + 4 * args.frag_sd < args.length:
                parser.error("--frag-mean + 4 --frag-sd lies below the read length: no fragment holds a read")
        try:
            parse_error_rate(args.error_rate)
        except ReadsError as e:
            parser.error(str(e))
        if prefix_refusal(args.prefix):
            parser.error(prefix_refusal(args.prefix))
    if args.quiet:
        args.ignore_warnings = True
        args.no_progress = True
    return add_outfile_names(args)
