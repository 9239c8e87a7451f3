"""python -m longcalld_amd.cli call ref.fa in.bam [region ...] -- the reference's command line (src/call_var_main.c:812-1000) for what the library supports: a thin
argument parser over lcd_call_files.  What is not supported is refused with one line and exit status 2."""
import sys

VERSION_FALLBACK = "longcalld_amd"
REFUSED = {
    "-s": "somatic / mosaic calling is not supported", "--mosaic": "somatic / mosaic calling is not supported", "--somatic": "somatic / mosaic calling is not supported",
    "--refine-aln": "--refine-aln is not supported: ask for refined alignments in the output BAM with --refine-bam", "-L": "-L/--input-is-list is not supported: give the list of input files with --bam-list FILE", "--input-is-list": "-L/--input-is-list is not supported: give the list of input files with --bam-list FILE",
    "-X": "-X/--extra-bam is not supported: give further input files with --add-bam FILE", "--extra-bam": "-X/--extra-bam is not supported: give further input files with --add-bam FILE",
    "-S": "-S/--out-sam is not supported: ask for SAM text with --sam FILE", "--out-sam": "-S/--out-sam is not supported: ask for SAM text with --sam FILE",
    "--out-cram": "CRAM output (-C FILE) is not supported: use -b or --sam",
    "-T": "-T/--trans-elem is not supported: give the TE sequence file with --te-lib FILE", "--trans-elem": "-T/--trans-elem is not supported: give the TE sequence file with --te-lib FILE",
    "--out-var-rnames": "--out-var-rnames is not supported: ask for the supporting read names of every record with --var-rnames",
    "--out-sv-rnames": "--out-sv-rnames is not supported: ask for the supporting read names of SV records with --sv-rnames",
    "--out-som-var-rnames": "--out-som-var-rnames is not supported: somatic / mosaic calling is not supported",
    "-m": "-m/--methylation is not supported (the reference reads no MM/ML tag behind it): ask for the per-haplotype CpG methylation table with --mods FILE",
    "--methylation": "-m/--methylation is not supported (the reference reads no MM/ML tag behind it): ask for the per-haplotype CpG methylation table with --mods FILE",
}
FLAGS = {"--make-index", "--hifi", "--ont", "--autosome-XY", "--autosome", "--all-ctg", "-H", "--no-vcf-header", "--amb-base", "--no-overlap", "--overlap", "--sort-merged", "--var-rnames", "--sv-rnames", "--refine-bam", "--mod-combine-strands", "--depth-skip-dels", "--split-gz", "--split-comment"}
VALUED = {"--region-file": "region_file", "--regions-file": "region_file", "-E": "exclude", "--exclude-ctg": "exclude", "-r": "ref_idx", "--ref-idx": "ref_idx",
          "-n": "sample_name", "--sample-name": "sample_name", "-o": "out_vcf", "--out-vcf": "out_vcf", "-O": "out_type", "--out-type": "out_type", "-l": "min_sv_len",
          "--min-sv-len": "min_sv_len", "-b": "out_bam", "--out-bam": "out_bam", "-c": "min_cov", "--min-cov": "min_cov", "-d": "alt_cov", "--alt-cov": "alt_cov",
          "-a": "alt_ratio", "--alt-ratio": "alt_ratio", "-M": "min_mapq", "--min-mapq": "min_mapq", "-B": "min_bq", "--min-bq": "min_bq", "-C": "max_cov", "--max-cov": "max_cov",
          "--window-chunks": "window_chunks", "--loader-threads": "loader_threads", "--chunk-len": "chunk_len", "--add-bam": "add_bam", "--bam-list": "bam_list", "--te-lib": "te_lib", "--sam": "out_sam", "--vcf-index": "vcf_index",
          "--mods": "mods", "--mod-code": "mod_code", "--mod-threshold": "mod_threshold", "--depth": "depth", "--depth-window": "depth_window", "--split-reads": "split_reads",
          "--haplotag-list": "haplotag_list"}
# haplotag: what `call` takes and it does not (no VCF is written, nothing is called), and its own options
HAPLOTAG_REFUSED = {k: "a haplotag run writes no VCF and calls no variants: %s is not one of its options" % k for k in (
    "-o", "--out-vcf", "-O", "--out-type", "--vcf-index", "--refine-bam", "--te-lib", "--var-rnames", "--sv-rnames", "-c", "--min-cov", "-d", "--alt-cov", "-a", "--alt-ratio",
    "-C", "--max-cov", "-l", "--min-sv-len", "-n", "--sample-name", "-H", "--no-vcf-header", "--amb-base")}
HAPLOTAG_FLAGS = {"--tag-snvs-only"}
HAPLOTAG_VALUED = {"--vcf-sample": "vcf_sample", "--tag-max-indel": "tag_max_indel", "--tag-min-diff": "tag_min_diff"}
USAGE = """Usage: python -m longcalld_amd.cli call [options] ref.fa in.bam [region ...]
       python -m longcalld_amd.cli haplotag [options] ref.fa in.bam phased.vcf[.gz] [region ...]   carry the phasing of a VCF onto the reads of any BAM (below)
       python -m longcalld_amd.cli index in.bam [out.bai]     build in.bam.bai (or out.bai) on the device
       python -m longcalld_amd.cli index [--csi] in.vcf.gz [out]   build in.vcf.gz.tbi (--csi: .csi) on the device; BAM or VCF is decided by the file's content, not its name
       python -m longcalld_amd.cli faidx ref.fa               build ref.fa.fai
  ref.fa needs ref.fa.fai, every input BAM needs its .bai; a missing one is an error unless --make-index is given
Inputs:   one sample from several BAMs (one per SMRT cell / flow cell, same reference table): --add-bam FILE (repeatable)   --bam-list FILE (one path per line)
          order: in.bam, the list's lines, the --add-bam files; the output BAM holds every input's records, file by file per chunk; --sort-merged orders them by
          position (and lets --make-index write <out.bam>.bai)
Input:    --hifi (default) | --ont   --region-file FILE   --autosome-XY (default) | --autosome | --all-ctg   -E/--exclude-ctg STR (repeatable)   -r/--ref-idx FILE
Output:   -n/--sample-name STR   -o/--out-vcf FILE [stdout]   -O/--out-type v|z   -l/--min-sv-len INT   -H/--no-vcf-header   --amb-base   -b/--out-bam FILE
          --te-lib FILE   TE sequences (FASTA, plain or gzip; the reference's -T): SVs that look like their insertion get MEI and REPNAME=
          --var-rnames | --sv-rnames   the supporting read names of every record | of SV records as the FORMAT field ALTREADS (the reference's --out-var-rnames /
          --out-sv-rnames; --var-rnames wins)
          --sam FILE   the alignment output as SAM text instead of -b (FILE "-": stdout, then -o must name a file); the records are formatted on the device
          --refine-bam   with -b or --sam: every kept read is written with the alignment the caller arrived at (CIGAR, POS, NM / MD / cs; the reference's --refine-aln);
          without -b / --sam it has no effect; a rewrite can move POS, so the output may stop being sorted (then no <out.bam>.bai is written, and the reason is printed)
          --mods FILE   the per-haplotype CpG methylation table from the reads' MM / ML tags (5mC by default), piled up on the device with the haplotypes of this
                        run: one line per reference CpG site and strand with a call (chrom start end code strand n_all mod_all n_h1 mod_h1 n_h2 mod_h2 n_filtered);
                        works with or without -b / --sam
          --mod-code m|h [m]   --mod-threshold INT [204] (128 ... 255: a call counts when its probability byte, or that of no modification, reaches it)
          --mod-combine-strands   one line per CpG: the '-' site is added to the '+' site, strand "."
          --depth FILE   the per-haplotype depth track, counted on the device from the records as stored in the input (--refine-bam does not change it) with the
                        haplotypes of this run: one BED line per run of equal depth (chrom start end depth_all depth_h1 depth_h2 depth_unassigned); M, = and X
                        cover, D covers, N does not; works with or without -b / --sam and beside --mods
          --depth-window INT [0]   one line per window of INT positions ([k INT + 1, (k + 1) INT] on the contig, cut to the called regions) with the sums of
                        depth x positions (bases_all bases_h1 bases_h2 bases_unassigned); 0: per base; at most 2^30
          --depth-skip-dels   a D does not cover
          --split-reads PREFIX   the reads of each haplotype as FASTQ, written on the device from the records with the haplotypes of this run: PREFIX.h1.fastq,
                        PREFIX.h2.fastq and PREFIX.none.fastq hold every primary record of the called regions once, in the order of the output BAM (a reverse-strand
                        record as it was sequenced; secondary and supplementary records are left out); works with or without -b / --sam
          --split-gz    with --split-reads: PREFIX.*.fastq.gz, BGZF-compressed on the device (valid gzip; `bgzip -r` can index it)
          --split-comment   with --split-reads: HP:i: and PS:i: behind the read name, tab-separated, where the output BAM carries the tag
          --haplotag-list FILE   one line per primary record: readname, H1 | H2 | none, the phase set or none, the contig (header #readname haplotype phaseset chromosome)
Calling:  -c/--min-cov INT   -d/--alt-cov INT   -a/--alt-ratio FLOAT   -M/--min-mapq INT   -B/--min-bq INT   -C/--max-cov INT
Index:    --make-index   build a missing .bai of any input / ref.fa.fai where it would have been read, and write <out.bam>.bai with -b (existing indexes are never touched; --sam gets no index);
                         it does not index the VCF: that is --vcf-index
          --vcf-index tbi|csi   with -O z and -o FILE: write FILE.tbi / FILE.csi beside the compressed VCF (built on the device from the text being compressed)
Run:      --window-chunks INT   --no-overlap (default) | --overlap   --loader-threads INT   --chunk-len INT
Haplotag: every read of in.bam is compared on the device with the heterozygous phased sites (GT a|b, PS) of phased.vcf -- SNVs and indels up to --tag-max-indel --
          and gets the haplotype most of its sites vote for; no variant is called and no VCF is written.  It takes the input, region, index and run options of
          `call`, -M, -B (the base quality an SNV base needs to vote), and the outputs that hang on the reads' haplotypes: -b | --sam, --sort-merged, --add-bam,
          --bam-list, --mods ..., --depth ..., --split-reads ..., --haplotag-list; at least one of them.  Its own options:
          --vcf-sample STR [the first]   --tag-snvs-only   --tag-max-indel INT [50]   --tag-min-diff INT [1] (votes the winning haplotype must lead by)
          Refused (exit status 2): -o, -O, --vcf-index, --refine-bam, --te-lib, --var-rnames, --sv-rnames, -n, -H, --amb-base and the calling thresholds -c -d -a -C -l
Not supported (refused with exit status 2): -s, --refine-aln (use --refine-bam), -L (use --bam-list), -X (use --add-bam), -T (use --te-lib), -S (use --sam), -C FILE, --out-var-rnames (use --var-rnames), --out-sv-rnames (use --sv-rnames),
          --out-som-var-rnames, -m/--methylation (use --mods FILE)
"""


def refuse(msg, cmd="call"):
    sys.stderr.write("longcalld_amd " + cmd + ": " + msg + "\n")
    return 2


def parse(argv, haplotag=False):
    """-> (dict of options, positional arguments) or an int exit status; haplotag: that command's options and refusals on top of `call`'s"""
    if haplotag:
        REFUSED, FLAGS, VALUED = dict(globals()["REFUSED"], **HAPLOTAG_REFUSED), globals()["FLAGS"] | HAPLOTAG_FLAGS, dict(globals()["VALUED"], **HAPLOTAG_VALUED)
        refuse = lambda msg: globals()["refuse"](msg, "haplotag")
    else:
        REFUSED, FLAGS, VALUED, refuse = globals()["REFUSED"], globals()["FLAGS"], globals()["VALUED"], globals()["refuse"]
    o = dict(flags=set(), exclude=[], add_bam=[])
    pos, i = [], 0
    while i < len(argv):
        a = argv[i]; i += 1
        if a == "--":
            pos += argv[i:]; break
        if a in ("-h", "--help"):
            sys.stdout.write(USAGE); return 0
        key, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") else (a, None)
        if len(a) > 2 and a[0] == "-" and a[1] != "-" and a[:2] in VALUED:           # -o out.vcf written as -oout.vcf
            key, val = a[:2], a[2:]
        if key in REFUSED:
            return refuse(REFUSED[key])
        if key in FLAGS:
            o["flags"].add(key); continue
        if key in VALUED:
            if val is None:
                if i >= len(argv):
                    return refuse(f"{key} needs a value")
                val = argv[i]; i += 1
            if VALUED[key] == "max_cov" and not val.lstrip("+").isdigit():
                return refuse(REFUSED["--out-cram"])
            if VALUED[key] in ("exclude", "add_bam"):
                o[VALUED[key]].append(val)
            else:
                o[VALUED[key]] = val
            continue
        if a.startswith("-") and a != "-":
            return refuse(f"unknown option {a}")
        pos.append(a)
    return o, pos


def vcf_fields(o):
    """--te-lib FILE / --var-rnames / --sv-rnames -> the keywords te_fasta= / rnames= of align.call_file (the reference's `output_var_rnames || (is_sv &&
    output_sv_rnames)`, src/vcf_utils.c:208: --var-rnames wins)"""
    return dict(te_fasta=o.get("te_lib"), rnames="all" if "--var-rnames" in o["flags"] else "sv" if "--sv-rnames" in o["flags"] else None)


def mods_option(o):
    """--mods FILE / --mod-code / --mod-threshold / --mod-combine-strands -> the keyword mods= of align.call_file (None without --mods), or the refusal's text"""
    extra = [k for k, name in (("mod_code", "--mod-code"), ("mod_threshold", "--mod-threshold")) if k in o] + (["x"] if "--mod-combine-strands" in o["flags"] else [])
    if "mods" not in o:
        return "--mod-code / --mod-threshold / --mod-combine-strands need --mods FILE" if extra else None
    if o["mods"] in ("", "-"):
        return "--mods needs a file: the table does not go to stdout"
    if o.get("mod_code", "m") not in ("m", "h"):
        return "--mod-code can only be m or h"
    try:
        thr = int(o.get("mod_threshold", 204))
    except ValueError:
        return "--mod-threshold is not a number"
    if not 128 <= thr <= 255:
        return "--mod-threshold must be 128 ... 255"
    return dict(path=o["mods"], code=o.get("mod_code", "m"), threshold=thr, combine_strands="--mod-combine-strands" in o["flags"])


def depth_option(o):
    """--depth FILE / --depth-window INT / --depth-skip-dels -> the keyword depth= of align.call_file (None without --depth), or the refusal's text"""
    if "depth" not in o:
        return "--depth-window / --depth-skip-dels need --depth FILE" if "depth_window" in o or "--depth-skip-dels" in o["flags"] else None
    if o["depth"] in ("", "-"):
        return "--depth needs a file: the track does not go to stdout"
    try:
        win = int(o.get("depth_window", 0))
    except ValueError:
        return "--depth-window is not a number"
    if not 0 <= win <= 1 << 30:
        return "--depth-window must be 0 ... 2^30"
    if o["depth"] == o.get("mods"):
        return "--depth and --mods name one file"
    return dict(path=o["depth"], window=win, skip_dels="--depth-skip-dels" in o["flags"])


def split_option(o):
    """--split-reads PREFIX / --split-gz / --split-comment / --haplotag-list FILE -> the keyword split= of align.call_file (None without --split-reads and
    --haplotag-list), or the refusal's text.  Refused: the two flags without --split-reads, an empty prefix or path, "-", and one of the four files equal to
    another output of the run (-o, -b / --sam, --mods, --depth, or each other)"""
    gz, comment = "--split-gz" in o["flags"], "--split-comment" in o["flags"]
    if "split_reads" not in o and (gz or comment):
        return "--split-gz / --split-comment need --split-reads PREFIX"
    if "split_reads" not in o and "haplotag_list" not in o:
        return None
    if o.get("split_reads") in ("", "-"):
        return "--split-reads needs a prefix: the read sets do not go to stdout"
    if o.get("haplotag_list") in ("", "-"):
        return "--haplotag-list needs a file: the list does not go to stdout"
    mine = [o["split_reads"] + s + (".fastq.gz" if gz else ".fastq") for s in (".none", ".h1", ".h2")] if "split_reads" in o else []
    mine += [o["haplotag_list"]] if "haplotag_list" in o else []
    others = [o[k] for k in ("out_vcf", "out_bam", "out_sam", "mods", "depth") if o.get(k) not in (None, "", "-")]
    if len(set(mine + others)) != len(mine + others):
        return "--split-reads / --haplotag-list: two outputs of the run name one file"
    return dict(prefix=o.get("split_reads"), gz=gz, comment=comment, haplotag_list=o.get("haplotag_list"))


def input_bams(o, bam):
    """the input files in order: the positional BAM, the lines of --bam-list (blank lines skipped; the reference likewise puts list entries before -X files), the
    --add-bam files"""
    bams = [bam]
    if "bam_list" in o:
        with open(o["bam_list"]) as f:
            bams += [ln.strip() for ln in f if ln.strip()]
    return bams + list(o["add_bam"])


def parse_index(argv):
    """index [--csi] FILE [OUT] | faidx ref.fa -> (command, paths) or an int exit status; `index --csi` comes back as the command index-csi"""
    cmd, rest = argv[0], argv[1:]
    if any(a in ("-h", "--help") for a in rest):
        sys.stdout.write(USAGE); return 0
    if cmd == "index" and "--csi" in rest:
        cmd, rest = "index-csi", [a for a in rest if a != "--csi"]
    bad = [a for a in rest if a.startswith("-") and a != "-"]
    if bad:
        return refuse(f"unknown option {bad[0]}")
    if (cmd.startswith("index") and len(rest) not in (1, 2)) or (cmd == "faidx" and len(rest) != 1):
        sys.stderr.write(USAGE); return 2
    return cmd, rest


def file_kind(path):
    """"bam" / "vcf" / None by the file's content, not its name: the start of the first gzip member (BGZF or not), inflated on the host (a few kilobytes), or of
    the file itself when it is not compressed.  None: neither "BAM\\1" nor "##fileformat=VCF" (or unreadable): `index` treats it as before, as a BAM"""
    import zlib
    try:
        with open(path, "rb") as f:
            head = f.read(1 << 16)
        text = zlib.decompressobj(31).decompress(head, 64) if head[:2] == b"\x1f\x8b" else head[:64]
    except (OSError, zlib.error):
        return None
    return "bam" if text[:4] == b"BAM\x01" else "vcf" if text.startswith(b"##fileformat=VCF") else None


def main_index(argv):
    p = parse_index(argv)
    if isinstance(p, int):
        return p
    cmd, paths = p
    from . import align
    try:
        if cmd.startswith("index"):
            kind = file_kind(paths[0])
            if cmd == "index-csi" and kind == "bam":
                return refuse("index --csi: only BAI is built for a BAM, not CSI")
            if cmd == "index-csi" and kind is None:
                return refuse("index --csi: the file is not a VCF")
            if kind != "vcf":
                st = align.bai_build(paths[0], paths[1] if len(paths) > 1 else None)
                sys.stderr.write(f"longcalld_amd index: {st['n_records']} records ({st['n_no_coor']} without coordinate), {st['n_slabs']} slabs, {st['ms_wall'] / 1000:.2f} s\n")
            else:       # VCF text; uncompressed or plain gzip, the builder refuses it with a message that says which of the two it is
                st = align.vcf_index_build(paths[0], paths[1] if len(paths) > 1 else None, fmt="csi" if cmd == "index-csi" else "tbi")
                sys.stderr.write(f"longcalld_amd index: {st['n_data_lines']} data lines on {st['n_contigs']} contigs, {st['n_slabs']} slabs, {st['ms_wall'] / 1000:.2f} s\n")
        else:
            n = align.fai_build(paths[0])
            sys.stderr.write(f"longcalld_amd faidx: {n} sequences\n")
    except align.LcdError as e:
        sys.stderr.write(f"longcalld_amd {cmd.split('-')[0]}: {e}\n")
        return 1
    return 0


def main_haplotag(argv):
    """haplotag [options] ref.fa in.bam phased.vcf[.gz] [region ...]: a thin parser over align.haplotag_file(s)"""
    no = lambda msg: refuse(msg, "haplotag")
    p = parse(argv, haplotag=True)
    if isinstance(p, int):
        return p
    o, pos = p
    if len(pos) < 3:
        sys.stderr.write(USAGE); return 2
    fasta, bam, vcf, regions = pos[0], pos[1], pos[2], pos[3:]
    if "ref_idx" in o and o["ref_idx"] != fasta + ".fai":
        return no("-r/--ref-idx: only <ref.fa>.fai next to the FASTA is supported")
    try:
        num = {k: int(o[k]) for k in ("min_mapq", "min_bq", "window_chunks", "loader_threads", "chunk_len", "tag_max_indel", "tag_min_diff") if k in o}
    except ValueError as e:
        return no(f"not a number: {e}")
    if num.get("tag_max_indel", 50) < 1:
        return no("--tag-max-indel must be at least 1")
    if num.get("tag_min_diff", 1) < 1:
        return no("--tag-min-diff must be at least 1")
    if not 0 <= num.get("min_bq", 0) <= 254:
        return no("-B/--min-bq must be 0 ... 254")
    if "out_sam" in o and "out_bam" in o:
        return no("--sam cannot be combined with -b/--out-bam: one alignment output per run")
    for f in (mods_option, depth_option, split_option):
        if isinstance(f(o), str):
            return no(f(o))
    mods, depth, split = mods_option(o), depth_option(o), split_option(o)
    sam = "out_sam" in o
    if not sam and "out_bam" not in o and mods is None and depth is None and split is None:
        return no("no output: give -b, --sam, --mods, --depth, --split-reads or --haplotag-list")
    from . import align
    cmdline = "longcalld_amd haplotag " + " ".join(argv)
    bam_out = dict(path=o["out_sam" if sam else "out_bam"], pg_line="@PG\tID:longcalld_amd\tPN:longcalld_amd\tCL:" + cmdline) if sam or "out_bam" in o else None
    try:
        bams = input_bams(o, bam)
    except OSError as e:
        return no(f"--bam-list: {e}")
    if len(bams) > 64:
        return no("more than 64 input files")
    mode = 2 if "--all-ctg" in o["flags"] else 1 if "--autosome" in o["flags"] else 0
    kw = dict(contig_mode=mode, exclude=o["exclude"], regions=regions, region_bed_path=o.get("region_file"), chunk_len=num.get("chunk_len", 0), window_chunks=num.get("window_chunks", 0),
              overlap=0 if "--no-overlap" in o["flags"] else 1 if "--overlap" in o["flags"] else -1, loader_threads=num.get("loader_threads", 0), min_mapq=num.get("min_mapq", 30),
              bam_out=bam_out, cfg=align.call_cfg(1 if "--ont" in o["flags"] else 0), index=(dict(build_missing_bai=1, build_missing_fai=1) if sam else True) if "--make-index" in o["flags"] else None,
              sample=o.get("vcf_sample"), max_indel=num.get("tag_max_indel", 50), snvs_only="--tag-snvs-only" in o["flags"], min_bq=num.get("min_bq", 0), min_diff=num.get("tag_min_diff", 1),
              **(dict(aln_format="sam") if sam else {}), **(dict(mods=mods) if mods is not None else {}), **(dict(depth=depth) if depth is not None else {}),
              **(dict(split=split) if split is not None else {}))
    try:
        st = align.haplotag_file(bam, fasta, vcf, **kw) if len(bams) == 1 else align.haplotag_files(bams, fasta, vcf, sort_output="--sort-merged" in o["flags"], **kw)
    except align.LcdError as e:
        sys.stderr.write(f"longcalld_amd haplotag: {e}\n")
        return 1
    if st.get("index", {}).get("out_bai_skipped"):
        sys.stderr.write("longcalld_amd haplotag: the output BAM was written without an index: " + st["index"]["out_bai_skip_reason"] + "\n")
    if st["plan_fallback"]:
        sys.stderr.write("longcalld_amd haplotag: no contig of the requested kind (or no valid region): the entire alignment file was processed\n")
    t, v = st["haplotag"], st["phased_vcf"]
    sys.stderr.write(f"longcalld_amd haplotag: {v['n_sites']} phased sites in {v['n_phase_sets']} sets ({v['n_lines'] - v['n_sites']} lines left out), {st['n_planned']} chunks, "
                     f"{st['n_reads']} reads: {t['n_tagged'][1]} H1 + {t['n_tagged'][2]} H2 + {t['n_tagged'][0]} untagged (records counted once per chunk that holds them), "
                     f"{st['ms_wall'] / 1000:.2f} s\n")
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        sys.stdout.write(USAGE); return 0 if argv else 2
    if argv[0] in ("index", "faidx"):
        return main_index(argv)
    if argv[0] == "haplotag":
        return main_haplotag(argv[1:])
    if argv[0] != "call":
        return refuse(f"unknown command {argv[0]} (the commands are: call, haplotag, index, faidx)")
    p = parse(argv[1:])
    if isinstance(p, int):
        return p
    o, pos = p
    if len(pos) < 2:
        sys.stderr.write(USAGE); return 2
    fasta, bam, regions = pos[0], pos[1], pos[2:]
    if o.get("out_type", "v") not in ("v", "z"):
        return refuse("-O/--out-type can only be v or z")
    if "ref_idx" in o and o["ref_idx"] != fasta + ".fai":
        return refuse("-r/--ref-idx: only <ref.fa>.fai next to the FASTA is supported")
    try:
        num = {k: int(o[k]) for k in ("min_sv_len", "min_cov", "alt_cov", "min_mapq", "min_bq", "max_cov", "window_chunks", "loader_threads", "chunk_len") if k in o}
        if "alt_ratio" in o:
            num["alt_ratio"] = float(o["alt_ratio"])
    except ValueError as e:
        return refuse(f"not a number: {e}")
    if "out_sam" in o and "out_bam" in o:
        return refuse("--sam cannot be combined with -b/--out-bam: one alignment output per run")
    if "vcf_index" in o:
        if o["vcf_index"] not in ("tbi", "csi"):
            return refuse("--vcf-index can only be tbi or csi")
        if o.get("out_type") != "z" or o.get("out_vcf", "-") == "-":
            return refuse("--vcf-index needs -O z and -o FILE: only a compressed VCF that goes to a file can be indexed")
    if o.get("out_sam") == "-" and o.get("out_vcf", "-") == "-":
        return refuse("--sam - needs -o FILE: the SAM text and the VCF cannot both go to stdout")
    mods = mods_option(o)
    if isinstance(mods, str):
        return refuse(mods)
    depth = depth_option(o)
    if isinstance(depth, str):
        return refuse(depth)
    split = split_option(o)
    if isinstance(split, str):
        return refuse(split)
    from . import align
    is_ont = 1 if "--ont" in o["flags"] else 0
    clean, opt, pass_, call = {}, {}, {}, {}
    if "min_cov" in num:
        clean["min_dp"] = opt["min_dp"] = call["min_dp"] = num["min_cov"]
    if "alt_cov" in num:
        clean["min_alt_dp"] = call["min_alt_dp"] = num["alt_cov"]
    if "alt_ratio" in num:
        clean["min_af"] = opt["min_af"] = num["alt_ratio"]
    if "min_bq" in num:
        clean["min_bq"] = num["min_bq"]
    if "min_sv_len" in num:
        clean["min_sv_len"] = opt["min_sv_len"] = call["min_sv_len"] = num["min_sv_len"]
    if "max_cov" in num:
        pass_["max_noisy_reg_cov"] = num["max_cov"]
    if "--amb-base" in o["flags"]:
        call["out_amb_base"] = 1
    cfg = align.call_cfg(is_ont, clean=clean, opt=opt, pass_=pass_, call=call)
    mode = 2 if "--all-ctg" in o["flags"] else 1 if "--autosome" in o["flags"] else 0
    cmdline = "longcalld_amd call " + " ".join(argv[1:])
    sam = "out_sam" in o
    bam_out = dict(path=o["out_sam" if sam else "out_bam"], pg_line="@PG\tID:longcalld_amd\tPN:longcalld_amd\tCL:" + cmdline) if sam or "out_bam" in o else None
    refine = "--refine-bam" in o["flags"]
    if refine and any(v is not None for v in vcf_fields(o).values()):
        return refuse("--refine-bam cannot be combined with --te-lib / --var-rnames / --sv-rnames in one run")
    try:
        bams = input_bams(o, bam)
    except OSError as e:
        return refuse(f"--bam-list: {e}")
    if len(bams) > 64:
        return refuse("more than 64 input files")
    run = align.call_file if len(bams) == 1 else (lambda _b, fa, **kw: align.call_files(bams, fa, sort_output="--sort-merged" in o["flags"], **kw))
    try:
        st = run(bam, fasta, contig_mode=mode, exclude=o["exclude"], regions=regions, region_bed_path=o.get("region_file"), chunk_len=num.get("chunk_len", 0),
                             window_chunks=num.get("window_chunks", 0), overlap=0 if "--no-overlap" in o["flags"] else 1 if "--overlap" in o["flags"] else -1, loader_threads=num.get("loader_threads", 0),
                             min_mapq=num.get("min_mapq", 30), vcf_path=o.get("out_vcf"), vcf_bgzf=1 if o.get("out_type") == "z" else 0,
                             no_vcf_header=1 if o["flags"] & {"-H", "--no-vcf-header"} else 0, sample_name=o.get("sample_name"), cmdline=cmdline, bam_out=bam_out, cfg=cfg,
                             index=(dict(build_missing_bai=1, build_missing_fai=1) if sam else True) if "--make-index" in o["flags"] else None,
                             **(dict(aln_format="sam") if sam else {}), **(dict(refine=True) if refine else vcf_fields(o)),
                             **(dict(vcf_index=o["vcf_index"]) if "vcf_index" in o else {}), **(dict(mods=mods) if mods is not None else {}),
                             **(dict(depth=depth) if depth is not None else {}), **(dict(split=split) if split is not None else {}))
    except align.LcdError as e:
        sys.stderr.write(f"longcalld_amd call: {e}\n")
        return 2 if "error -2:" in str(e) else 1
    if st.get("index", {}).get("out_bai_skipped"):
        sys.stderr.write("longcalld_amd call: the output BAM was written without an index: " + st["index"]["out_bai_skip_reason"] + "\n")
    if st.get("vcf_index", {}).get("skipped"):
        sys.stderr.write("longcalld_amd call: the VCF was written without an index: " + st["vcf_index"]["skip_reason"] + "\n")
    if st["plan_fallback"]:
        sys.stderr.write("longcalld_amd call: no contig of the requested kind (or no valid region): the entire alignment file was processed\n")
    per_file = f" ({' + '.join(str(x) for x in st['n_reads_per_file'])} from the {len(bams)} input files)" if len(bams) > 1 else ""
    sys.stderr.write(f"longcalld_amd call: {st['n_planned']} chunks in {st['n_windows']} windows, {st['n_reads']} reads{per_file}, {st['n_vcf_lines']} VCF lines, "
                     + (f"{st['n_mei_lines']} MEI records, " if "n_mei_lines" in st else "")
                     + (f"{st['refine']['n_refined']} refined / {st['refine']['n_unrefined']} unrefined records, " if refine and bam_out is not None else "")
                     + (f"{st['bam_out']['bytes_file']} bytes of SAM text, " if sam else "") + (f"{st['mods']['n_rows']} methylation rows, " if mods is not None else "")
                     + (f"{st['depth']['n_rows']} depth rows, " if depth is not None else "")
                     + (f"{st['split']['n_hap'][1]} + {st['split']['n_hap'][2]} + {st['split']['n_hap'][0]} split reads, " if split is not None else "")
                     + f"{st['ms_wall'] / 1000:.2f} s\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
