"""``mutation-simulator file {args,rmt,it}`` (reference __main__.py:34-111) on an MI355X, plus ``file vcf truth.vcf``
(``--consensus``: any VCF, one haplotype of one sample), ``file profile calls.vcf`` (the VCF's SBS-96 spectrum, counted
against the reference), ``file compare truth.vcf calls.vcf`` (the calls scored against the truth) and ``file reads -n N``
(FASTQ reads drawn from the genome)."""
from __future__ import annotations

import json
import random
import sys
from timeit import default_timer as timer

from . import *  # noqa: F401,F403  (same style of namespace as the reference entry point)
from ._ffi import MsimError, MsimUnsupported
from .argument_parser import compare_refusal, ploidy_refusal, profile_refusal, reads_refusal, spectrum_refusal
from .spectrum import SpectrumError
from .fasta_io import is_gzip

_INIT_ERRORS = (FileNotFoundError, ITNotEnoughAvailChromsError, RatesTooHighError, RatesTooLowError,
                FastaIndexingError, FastaNotFoundError, ItRateTooHighError, ItRateTooLowError,
                RMTParseError, MissingLengthError, MinimumLengthTooLowError, TitvTooLowError,
                ChromNotExistError, RangeDefinitionOutOfBoundsError, FastaDuplicateHeaderError,
                MinimumLengthHigherThanMaximumError, UnsupportedCompressionFormat)


STAGES: dict = {}          # wall seconds of the last run's stages (--bench-json: cli_s)


class BgzipUnsupportedError(Exception):
    """--bgzip together with what it does not cover (the IT pass, a sharded run)."""


class VcfModeUnsupportedError(Exception):
    """The vcf mode together with what it does not cover (a sharded run)."""


class ChainUnsupportedError(Exception):
    """--chain together with what it does not cover (the IT pass, a sharded run)."""


class PloidyUnsupportedError(Exception):
    """--ploidy 2 together with what it does not cover (argument_parser.ploidy_refusal)."""


class SpectrumUnsupportedError(Exception):
    """--spectrum together with what it does not cover (argument_parser.spectrum_refusal)."""


class ProfileUnsupportedError(Exception):
    """The profile mode together with what it does not cover (argument_parser.profile_refusal)."""


class CompareUnsupportedError(Exception):
    """The compare mode together with what it does not cover (argument_parser.compare_refusal)."""


class ReadsUnsupportedError(Exception):
    """The reads mode together with what it does not cover (argument_parser.reads_refusal)."""


class CompressedInputUnsupportedError(Exception):
    """A gzip-compressed input together with what does not cover it (a sharded run)."""


def _warm_up(args):
    try:
        from ._ffi import warm_up_async
        warm_up_async(args.device or 0, pin=True)
    except Exception:  # noqa: BLE001  (no library: Mutator reports it properly)
        pass


def initialize(argv=None):
    t0 = timer()
    args = get_args(argv)
    STAGES["parse_args"] = timer() - t0
    refusal = profile_refusal(args)
    if refusal:
        exit_with_error(ProfileUnsupportedError(refusal), args.no_color)
    refusal = compare_refusal(args)
    if refusal:
        exit_with_error(CompareUnsupportedError(refusal), args.no_color)
    refusal = reads_refusal(args)
    if refusal:
        exit_with_error(ReadsUnsupportedError(refusal), args.no_color)
    refusal = ploidy_refusal(args)
    if refusal:
        exit_with_error(PloidyUnsupportedError(refusal), args.no_color)
    refusal = spectrum_refusal(args)
    if refusal:
        exit_with_error(SpectrumUnsupportedError(refusal), args.no_color)
    if getattr(args, "spectrum", None) is not None:    # (read before the GPU comes up: a file that cannot be used ends the run here)
        from .spectrum import load as load_spectrum
        try:
            args.spectrum_weights = load_spectrum(args.spectrum, args.signature)
        except SpectrumError as e:
            exit_with_error(e, args.no_color)
    if args.mode == "vcf" and (args.gpus or 1) > 1:
        exit_with_error(VcfModeUnsupportedError("the vcf mode needs a single-GPU run (--gpus 1)"), args.no_color)
    if args.bgzip and args.mode == "it":
        exit_with_error(BgzipUnsupportedError("--bgzip does not apply to the interchromosomal pass (it)"), args.no_color)
    if args.bgzip and (args.gpus or 1) > 1:
        exit_with_error(BgzipUnsupportedError("--bgzip needs a single-GPU run (--gpus 1)"), args.no_color)
    if args.chain and args.mode == "it":
        exit_with_error(ChainUnsupportedError("--chain does not apply to the interchromosomal pass (it)"), args.no_color)
    if args.chain and (args.gpus or 1) > 1:
        exit_with_error(ChainUnsupportedError("--chain needs a single-GPU run (--gpus 1)"), args.no_color)
    if (args.gpus or 1) > 1 and is_gzip(args.infile):
        # (the parent of a sharded run never opens a GPU, and parent and workers would each inflate the whole file)
        exit_with_error(CompressedInputUnsupportedError(
            f"compressed input ({args.infile.name}) needs a single-GPU run (--gpus 1); inflate it first (bgzip -d) for --gpus N"),
            args.no_color)
    # the GPU comes up while the FASTA is read and indexed (never in the parent of --gpus N; with --bgzip and an RMT only
    # once the RMT is known to hold no it lines)
    early = (args.gpus or 1) <= 1 and not (args.bgzip and args.mode == "rmt")
    if early:
        _warm_up(args)
    try:
        t0 = timer()
        fasta = load_fasta(args.infile, args.device or 0)
        STAGES["load_index"] = timer() - t0
        # the genome's own name: what the VCF header and an RMT's `fasta` line call it (genome.fa for a BGZF genome.fa.gz)
        args.genome_name = args.infile.name
        if fasta.compressed and args.infile.suffix.lower() in (".gz", ".bgz") and args.infile.stem:
            args.genome_name = args.infile.stem
        if args.mode in ("vcf", "profile", "compare", "reads"):    # a replay, a profile, a comparison and the reads have no settings
            return args, fasta, None
        if args.mode == "args":
            sim = SimulationSettings.from_args(args, fasta, args.ignore_warnings)
        elif args.mode == "it":
            sim = SimulationSettings.from_it(args.interchromosomalrate, fasta, args.ignore_warnings)
        else:
            sim = SimulationSettings.from_rmt(args.rmtfile, fasta, args.ignore_warnings)
    except _INIT_ERRORS as e:
        exit_with_error(e, args.no_color)
    if args.bgzip and sim.has_it:
        exit_with_error(BgzipUnsupportedError("--bgzip does not apply to the interchromosomal pass (it lines in the RMT)"),
                        args.no_color)
    refusal = ploidy_refusal(args, sim.has_it)
    if refusal:
        exit_with_error(PloidyUnsupportedError(refusal), args.no_color)
    if args.chain and sim.has_it:
        exit_with_error(ChainUnsupportedError("--chain does not apply to the interchromosomal pass (it lines in the RMT)"),
                        args.no_color)
    if not early and (args.gpus or 1) <= 1:
        _warm_up(args)
    if not args.ignore_warnings:
        warn_user(args, sim)
    return args, fasta, sim


def warn_user(args, sim):
    if sim.fasta and sim.fasta not in (args.infile.name, getattr(args, "genome_name", args.infile.name)):
        print_warning("Fasta filename does not match RMT", args.no_color)
    if sim.md5 and get_md5(args.infile) != sim.md5:
        print_warning("Fasta md5 hash does not match RMT", args.no_color)


def main(argv=None):
    start = timer()
    args, fasta, sim = initialize(argv)
    loaded = timer()
    if args.mode == "vcf":                             # (--seed / --rng have no effect: no generator is touched)
        from .vcf_replay import VcfReplay, VcfReplayError
        try:
            replay = VcfReplay(args, fasta)
            try:
                replay.run()
            finally:
                replay.close()
            fasta.close()
            if args.bench_json:
                stats = dict(replay.stats)
                stats["cli_s"] = {"load_index": round(STAGES.get("load_index", 0.0), 4), "replay": round(timer() - loaded, 4)}
                args.bench_json.write_text(json.dumps(stats, indent=1) + "\n")
        except (FastaWriterError, ChainWriterError, VcfReplayError, MsimError, FileNotFoundError, UnsupportedCompressionFormat,
                ValueError) as e:
            exit_with_error(e, args.no_color)
        if not args.quiet:
            print_success(f"Mutation-Simulator finished in: {round(timer() - start, 4)}s", args.no_color)
        return
    if args.mode == "profile":                         # (--seed / --rng have no effect: no generator is touched)
        from .profile import Profile, ProfileError
        from .vcf_replay import VcfReplayError
        try:
            profile = Profile(args, fasta)
            try:
                profile.run()
            finally:
                profile.close()
            fasta.close()
            if args.bench_json:
                stats = dict(profile.stats)
                stats["cli_s"] = {"load_index": round(STAGES.get("load_index", 0.0), 4), "profile": round(timer() - loaded, 4)}
                args.bench_json.write_text(json.dumps(stats, indent=1) + "\n")
        except (ProfileError, SpectrumError, VcfReplayError, MsimError, OSError, UnsupportedCompressionFormat, ValueError) as e:
            exit_with_error(e, args.no_color)
        if not args.quiet:
            print_success(f"Mutation-Simulator finished in: {round(timer() - start, 4)}s", args.no_color)
        return
    if args.mode == "compare":                         # (--seed / --rng have no effect: no generator is touched)
        from .compare import Compare, CompareError
        from .vcf_replay import VcfReplayError
        try:
            compare = Compare(args, fasta)
            try:
                compare.run()
            finally:
                compare.close()
            fasta.close()
            if args.bench_json:
                stats = dict(compare.stats)
                stats["cli_s"] = {"load_index": round(STAGES.get("load_index", 0.0), 4), "compare": round(timer() - loaded, 4)}
                args.bench_json.write_text(json.dumps(stats, indent=1) + "\n")
        except (CompareError, VcfReplayError, MsimError, OSError, UnsupportedCompressionFormat, ValueError) as e:
            exit_with_error(e, args.no_color)
        if not args.quiet:
            print_success(f"Mutation-Simulator finished in: {round(timer() - start, 4)}s", args.no_color)
        return
    if args.mode == "reads":                           # (--seed is the Philox key; --rng has no effect: no mutation engine runs)
        from .reads import Reads, ReadsError
        try:
            reads = Reads(args, fasta)
            try:
                reads.run()
            finally:
                reads.close()
            fasta.close()
            if args.bench_json:
                stats = dict(reads.stats)
                stats["cli_s"] = {"load_index": round(STAGES.get("load_index", 0.0), 4), "reads": round(timer() - loaded, 4)}
                args.bench_json.write_text(json.dumps(stats, indent=1) + "\n")
        except (ReadsError, MsimError, OSError, UnsupportedCompressionFormat, ValueError) as e:
            exit_with_error(e, args.no_color)
        if not args.quiet:
            print_success(f"Mutation-Simulator finished in: {round(timer() - start, 4)}s", args.no_color)
        return
    if args.seed is not None:
        import numpy
        random.seed(args.seed)
        numpy.random.seed(args.seed)
    if sim.has_mutations:
        try:
            t0 = timer()
            mutator = Mutator(args, fasta, sim)
            t1 = timer()
            try:
                mutator.mutate()
            finally:
                t2 = timer()
                mutator.close()            # (also on the reference's KeyError / ValueError: the files are complete as far as they go)
            fasta.close()
            if args.bench_json:
                stats = dict(mutator.stats)
                from . import mutator as _m
                stats["replanned_contigs"] = _m.REPLANNED_CONTIGS     # device window overflows recovered on the host (expected: 0)
                if getattr(args, "spectrum", None) is not None:
                    stats["census_ms"], stats["spectrum_plan_ms"] = (round(x, 4) for x in mutator.spectrum_ms)
                stats["cli_s"] = {"load_index_settings": round(loaded - start, 4), "mutate_and_write": round(timer() - loaded, 4),
                                  "parse_args": round(STAGES.get("parse_args", 0.0), 4), "load_index": round(STAGES.get("load_index", 0.0), 4),
                                  "open_writers": round(t1 - t0, 4), "mutate": round(t2 - t1, 4), "close": round(timer() - t2, 4)}
                args.bench_json.write_text(json.dumps(stats, indent=1) + "\n")
        except (FastaWriterError, VcfWriterError, ChainWriterError, MsimError, SpectrumError) as e:
            exit_with_error(e, args.no_color)
    if sim.has_it:                         # the second pass reads what the first one wrote (reference __main__.py:88-102)
        if sim.has_mutations:
            try:
                fasta = load_fasta(args.outfasta, args.device or 0)
            except (FastaDuplicateHeaderError, FastaIndexingError, FastaNotFoundError, UnsupportedCompressionFormat) as e:
                exit_with_error(e, args.no_color)
        try:
            it_mutator = ITMutator(args, fasta, sim)
            try:
                it_mutator.mutate()
            finally:
                it_mutator.close()
            fasta.close()
        except (FastaWriterError, BedpeWriterError, MsimError) as e:
            exit_with_error(e, args.no_color)
    runtime = round(timer() - start, 4)
    if not args.quiet:
        print_success(f"Mutation-Simulator finished in: {runtime}s", args.no_color)


if __name__ == "__main__":
    main()
