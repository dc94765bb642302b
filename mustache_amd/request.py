"""What a run of `mustache` or `diff_mustache` may do: the one place that says no.

Each command line puts what it was asked into a Request and calls plan(), which returns the line of a refused run or the Plan
of one that goes ahead.  Every rule is stated here once, with its sentence once, and plan() applies them in ONE order, the same
for both command lines ("The order of refusals").  The guards of the library (mustache.read_contacts, read_sample,
diff_trans.regulate, pileup's trans mode, balance_genome.check_genome_request, trans.read_trans_contacts) raise their own
exception types with the rule functions and sentences of this module.  balance.check_request (`--balance`) and
balance_genome.check_genome_request (`--balance-genome`) are the two rules that live beside what they guard; the rule of
`--downsample` / `--seed` / `--match-depth` (thinning) is here, with the helpers of mustache_amd/downsample.py for P and the seed,
and so is the rule of `--downsample-genome` / `--match-depth-genome` (thinning_genome);
so is the rule of `--coarser` / `--merge-distance` (multires), with mustache_amd/multires.py's parse of the resolutions, and
that of `--coarser-genome` (multires_genome), the same for the whole genome's map under --balance-genome.

Host only: no torch and no native library at import; plan() reads no contact data except the one parse of a pairs file under
--pairs-trans (keep_trans_rows) and the chromosome list of a run without -ch."""
import os
from collections import namedtuple

from .balance import BalanceError, check_request

BALANCE_ON_TRANS = "--balance does not apply to inter-chromosomal pairs"
TEXT_ON_TRANS = "Interchromosomal analysis is only supported for .hic and .cool input formats."
ONE_GPU = "inter-chromosomal pairs run on one GPU only"
NEED_CH = "inter-chromosomal pairs need -ch and -ch2 (all-pairs runs are not supported)"
TRANS_ALL_CH2 = "--trans-all pairs the -ch list with itself; give -ch2 without it"
RAW_PAIRS = "%s holds raw read pairs: give --balance ICE|NEWTON"
THIN_INPUT = "%s and %s: raw counts are thinned from .hic and .pairs / .pairs.gz input only"

# files: the contact file(s), one or two (None: not given); bias: [(the -b / -b1 / -b2 file or None, the sentence when it is
# missing)]; bias_flag: the flag to quote; ch, ch2: the -ch / -ch2 lists ('n' when absent); ranks: the ranks of the run;
# text_pair_raises: a trans pair on text input ends the run as the reference's one-sample caller does (Raises)
_RequestTuple = namedtuple("Request", "files bias bias_flag norm_method balance balance_genome balance_pixels balance_pixels_given "
                                      "pairs_trans pairs_zero_based trans_all ch ch2 ranks text_pair_raises downsample seed match_depth",
                           defaults=(None, None, False))
# downsample: --downsample's fraction (None: not given); seed: --seed (None: not given); match_depth: diff_mustache's --match-depth


class Request(_RequestTuple):
    """The tuple above, and behind it -- by keyword only, with defaults -- what `mustache` asks of mustache_amd/multires.py:
    coarser = the --coarser strings (None: not given), merge_distance = --merge-distance (None: not given), coarser_genome =
    the --coarser-genome strings (None: not given); and what either
    command line asks of the genome thinning: downsample_genome = --downsample-genome's fraction (None: not given),
    match_depth_genome = diff_mustache's --match-depth-genome.  They are attributes beside the tuple, not fields of it:
    tests/test_cli_downsample_requests.py pins the tuple's last three fields, and a positional caller keeps working either way."""
    EXTRA = ("coarser", "merge_distance", "downsample_genome", "match_depth_genome", "coarser_genome")

    def __new__(cls, *fields, coarser=None, merge_distance=None, downsample_genome=None, match_depth_genome=False,
                coarser_genome=None, **named):
        self = super().__new__(cls, *fields, **named)
        self.coarser, self.merge_distance, self.coarser_genome = coarser, merge_distance, coarser_genome
        self.downsample_genome, self.match_depth_genome = downsample_genome, bool(match_depth_genome)
        return self

    def _replace(self, **changes):
        extra = {k: changes.pop(k, getattr(self, k)) for k in self.EXTRA}
        return type(self)(*super()._replace(**changes), **extra)

# cis, trans: the (chromosome, chromosome2) pairs in run order, every cis pair before the first trans pair; trans_all: a
# --trans-all run; balance: the --balance method in upper case, or None; genome: --balance-genome's (method, pixels), or None
Plan = namedtuple("Plan", "cis trans trans_all balance genome")


def request_of(args, files, bias, bias_flag, ranks, text_pair_raises=False):
    """the Request of a command line's parsed arguments"""
    return Request(list(files), bias, bias_flag, args.norm_method, args.balance, args.balance_genome, args.balance_pixels,
                   args.balance_pixels_given, args.pairs_trans, args.pairs_zero_based, args.trans_all, args.chromosome,
                   args.chromosome2, ranks, text_pair_raises, args.downsample, args.seed, getattr(args, "match_depth", False),
                   coarser=getattr(args, "coarser", None), merge_distance=getattr(args, "merge_distance", None),
                   downsample_genome=getattr(args, "downsample_genome", None),
                   match_depth_genome=getattr(args, "match_depth_genome", False),
                   coarser_genome=getattr(args, "coarser_genome", None))


class Raises(str):
    """The sentence of a refusal that ends in an exception instead of a return: a trans pair on text input in `mustache`,
    where the reference prints and raises FileNotFoundError (mustache.py:869-871)."""
    error = FileNotFoundError


def refuse(why):
    """what a command line does with the string plan() returned"""
    print(why)
    if isinstance(why, Raises):
        raise why.error


# ----------------------------------------------------------------------------------------------------------------------
# the rules: the sentence of the conflict, or None
# ----------------------------------------------------------------------------------------------------------------------
def given_bias(rq):
    """the first bias file the request names, or None"""
    return next((path for path, _ in rq.bias if path), None)


def balance_on_trans(balance):
    return BALANCE_ON_TRANS if balance is not None else None


def trans_ranks(ranks, count=True):
    if ranks > 1:
        return ONE_GPU + (" (this run has %d ranks)" % ranks if count else "")
    return None


def trans_input(files, pairs_trans=False):
    """inter-chromosomal records come from `.hic`, `.cool` and `.mcool` files -- and, under --pairs-trans, from pairs files"""
    from .pairs import is_pairs
    if all(str(f).endswith((".hic", ".cool", ".mcool")) or (pairs_trans and is_pairs(f)) for f in files):
        return None
    return TEXT_ON_TRANS


def other_chromosome(ch, ch2):
    """does -ch2 name another chromosome than -ch somewhere (an inter-chromosomal pair, or lists that do not zip)?"""
    return isinstance(ch2, list) and (not isinstance(ch, list) or len(ch) != len(ch2) or any(a != b for a, b in zip(ch, ch2)))


def pairs_input(rq):
    """What pairs input (or --pairs-zero-based / --pairs-trans without one) rules out.  Reads nothing."""
    from .pairs import is_pairs
    files, ch, ch2 = rq.files, rq.ch, rq.ch2
    bias = given_bias(rq)
    mine = [f for f in files if is_pairs(f)]
    if not mine:
        if rq.pairs_trans:
            return "--pairs-trans is for .pairs / .pairs.gz input (%s is none)" % ", ".join(str(f) for f in files)
        if rq.pairs_zero_based:
            return "--pairs-zero-based is for .pairs / .pairs.gz input (%s is none)" % ", ".join(str(f) for f in files)
        return None
    other = other_chromosome(ch, ch2)
    if rq.pairs_trans:                       # the trans rows are kept for --balance-genome (balance_genome.py)
        if not rq.trans_all and not other:
            return "--pairs-trans on a run with no inter-chromosomal pair: give --trans-all, or -ch A -ch2 B"
        if rq.balance is not None or bias or (rq.norm_method and str(rq.norm_method).upper() != "NONE"):
            return "--pairs-trans with --balance, %s or -norm: the trans rows of %s are raw read pairs and are balanced with " \
                   "the whole genome; give --balance-genome ICE|NEWTON alone" % (rq.bias_flag, mine[0])
        if rq.balance_genome is None:
            return "--pairs-trans without --balance-genome: %s holds raw read pairs; give --balance-genome ICE|NEWTON" % mine[0]
        if rq.ranks > 1:
            return "--pairs-trans in a multi-rank run (world size %d): the genome is balanced on one GPU; start a single " \
                   "process" % rq.ranks
        return None
    without = "without --pairs-trans only intra-chromosomal loops are called from a pairs file"
    if rq.trans_all:
        return "--trans-all and %s: %s" % (mine[0], without)
    if rq.balance_genome is not None:
        return "--balance-genome and %s: %s; use --balance" % (mine[0], without)
    if other:
        return "-ch2 with another chromosome and %s: %s" % (mine[0], without)
    if rq.balance is None:
        return RAW_PAIRS % mine[0]
    try:
        check_request(rq.balance, files, bias, rq.norm_method, rq.ranks, bias_flag=rq.bias_flag)
    except BalanceError as e:
        return str(e)
    return None


def thinning(rq):
    """What --downsample / --match-depth / --seed (mustache_amd/downsample.py) rule out.  Reads nothing."""
    from .downsample import DownsampleError, check_seed, threshold_of
    from .pairs import is_pairs
    if rq.downsample is None and not rq.match_depth:
        if rq.seed is not None and rq.downsample_genome is None and not rq.match_depth_genome:
            return "--seed without --downsample or --match-depth: it seeds the thinning and nothing else"
        return None
    if rq.match_depth and rq.downsample is not None:
        return "--match-depth and --downsample: give one of them (--match-depth thins the deeper sample to the other's depth)"
    flag = "--match-depth" if rq.match_depth else "--downsample"
    try:
        if rq.downsample is not None:
            threshold_of(rq.downsample)
        if rq.seed is not None:
            check_seed(rq.seed)
    except DownsampleError as e:
        return str(e)
    if rq.trans_all or rq.balance_genome is not None or rq.pairs_trans or other_chromosome(rq.ch, rq.ch2):
        return "%s on a run with an inter-chromosomal pair: only intra-chromosomal maps are thinned" % flag
    if given_bias(rq) or (rq.norm_method and str(rq.norm_method).upper() != "NONE"):
        return "%s with %s or -norm: thinning needs raw integer counts; give --balance ICE|NEWTON alone" % (flag, rq.bias_flag)
    if rq.balance is None:
        return "%s without --balance: thinning needs raw integer counts; give --balance ICE|NEWTON" % flag
    for f in rq.files:
        if not (is_pairs(f) or str(f).endswith(".hic")):
            return THIN_INPUT % (flag, f)
    return None


def thinning_genome(rq):
    """What --downsample-genome / --match-depth-genome (the genome thinning of mustache_amd/downsample.py) rule out, before
    thinning(): the flags of one chromosome's thinning and these exclude each other.  What --balance-genome itself refuses --
    a run that is not all inter-chromosomal pairs, text / `.cool` input, several ranks, pairs input without --pairs-trans --
    keeps check_genome_request's and pairs_input's sentences.  Reads nothing."""
    from .downsample import DownsampleError, check_seed, threshold_of
    if rq.downsample_genome is None and not rq.match_depth_genome:
        return None
    flag = "--match-depth-genome" if rq.match_depth_genome else "--downsample-genome"
    if rq.balance_genome is None:
        return "%s without --balance-genome: thinning the genome's map needs raw integer counts; give --balance-genome " \
               "ICE|NEWTON" % flag
    if rq.match_depth_genome and rq.downsample_genome is not None:
        return "--match-depth-genome and --downsample-genome: give one of them (--match-depth-genome thins the deeper sample's " \
               "genome to the other's depth)"
    if rq.downsample is not None or rq.match_depth:
        return "%s and %s: give one of them (%s thins each chromosome's own map, %s the whole genome's)" \
               % (("--match-depth" if rq.match_depth else "--downsample", flag) * 2)
    if rq.match_depth_genome and len(rq.files) < 2:
        return "--match-depth-genome matches the depths of two samples: it is diff_mustache's"
    try:
        if rq.downsample_genome is not None:
            threshold_of(rq.downsample_genome, "--downsample-genome")
        if rq.seed is not None:
            check_seed(rq.seed)
    except DownsampleError as e:
        return str(e)
    return None


def genome_thinning_of(rq):
    """what mustache.genome_biases_or_error takes of an accepted request: (T, seed), ("match", seed) or None"""
    from .downsample import threshold_of
    if rq.match_depth_genome:
        return "match", int(rq.seed or 0)
    if rq.downsample_genome is not None:
        return threshold_of(rq.downsample_genome, "--downsample-genome"), int(rq.seed or 0)
    return None


def coarser_resolutions(rq, res):
    """the --coarser resolutions of the request in bp, ascending ([] without the flag); multires.MultiresError for a value
    the rule below refuses"""
    if rq.coarser is None:
        return []
    from .multires import parse_resolutions
    return parse_resolutions(int(res), rq.coarser)


def multires(rq, res):
    """What --coarser / --merge-distance (mustache_amd/multires.py) rule out at -r = res bp.  Reads nothing."""
    from .multires import NOT_RAW, MultiresError
    from .pairs import is_pairs
    if rq.coarser is None:
        if rq.merge_distance is not None and rq.coarser_genome is None:
            return "--merge-distance without --coarser: it is the tolerance of the multi-resolution merge and nothing else"
        return None
    if rq.merge_distance is not None and int(rq.merge_distance) < 0:
        return "--merge-distance %d: the distance is a number of bins >= 0" % rq.merge_distance
    try:
        coarser_resolutions(rq, res)
    except MultiresError as e:
        return str(e)
    if rq.trans_all or rq.balance_genome is not None or rq.pairs_trans or other_chromosome(rq.ch, rq.ch2):
        return "--coarser on a run with an inter-chromosomal pair: only intra-chromosomal maps are coarsened"
    if given_bias(rq) or (rq.norm_method and str(rq.norm_method).upper() != "NONE"):
        return "--coarser with %s or -norm: %s" % (rq.bias_flag, NOT_RAW)
    if rq.balance is None:
        return "--coarser without --balance: %s" % NOT_RAW
    for f in rq.files:
        if not (is_pairs(f) or str(f).endswith(".hic")):
            return "--coarser and %s: raw counts are coarsened from .hic and .pairs / .pairs.gz input only" % f
    if rq.ranks > 1:
        return "--coarser in a multi-rank run (world size %d): every resolution of a chromosome is called on one GPU; start a " \
               "single process" % rq.ranks
    return None


def coarser_genome_resolutions(rq, res):
    """the --coarser-genome resolutions of the request in bp, ascending ([] without the flag); multires.MultiresError for a
    value the rule below refuses"""
    if rq.coarser_genome is None:
        return []
    from .multires import parse_resolutions
    return parse_resolutions(int(res), rq.coarser_genome, flag="--coarser-genome")


def multires_genome(rq, res):
    """What --coarser-genome (the genome's coarsening of mustache_amd/multires.py) rules out at -r = res bp, before multires():
    the two flags exclude each other and share --merge-distance.  What --balance-genome itself refuses -- a run that is not
    all inter-chromosomal pairs, text / `.cool` input, several ranks, pairs input without --pairs-trans -- keeps
    check_genome_request's and pairs_input's sentences.  Reads nothing."""
    from .multires import MultiresError
    if rq.coarser_genome is None:
        return None
    if rq.coarser is not None:
        return "--coarser-genome and --coarser: give one of them (--coarser coarsens each chromosome's own map, " \
               "--coarser-genome the whole genome's)"
    if rq.balance_genome is None:
        return "--coarser-genome without --balance-genome: coarsening the genome's map sums raw integer counts; give " \
               "--balance-genome ICE|NEWTON"
    if rq.merge_distance is not None and int(rq.merge_distance) < 0:
        return "--merge-distance %d: the distance is a number of bins >= 0" % rq.merge_distance
    try:
        coarser_genome_resolutions(rq, res)
    except MultiresError as e:
        return str(e)
    return None


def keep_trans_rows(files, zero_based):
    """--pairs-trans: each pairs file's one parse of the run keeps the trans rows, whoever asks for the handle first, and
    happens here, before a GPU is touched: a file without `#chromsize` lines ends the run with the reader's sentence."""
    from .balance_genome import pairs_open
    from .pairs import is_pairs, want_trans
    for f in files:
        if is_pairs(f):
            want_trans(f)
            try:
                pairs_open(f, zero_based)
            except BalanceError as e:
                return str(e)
    return None


# ----------------------------------------------------------------------------------------------------------------------
# the pair lists
# ----------------------------------------------------------------------------------------------------------------------
def _all_chromosomes(f, res, pairs_zero_based):
    """every chromosome of a file that names them, for a run without -ch: readers.list_chromosomes, or a pairs file's table in
    table order (the one parse of the run: the handle stays cached for the reads that follow) -- or the Error: line of a pairs
    file the reader refuses"""
    from .pairs import is_pairs
    if not is_pairs(f):
        from .readers import list_chromosomes
        return list_chromosomes(f, res)
    from .hicfile import HicError
    from .pairs import list_chromosomes as pairs_chromosomes
    try:
        return pairs_chromosomes(f, pairs_zero_based)
    except HicError as e:
        return "Error: %s" % e


def chromosome_pairs(f, res, ch, ch2, pairs_zero_based=False):
    """-ch / -ch2 -> [(chromosome, chromosome2)] (without -ch: every chromosome of a `.hic` / `.cool` / `.mcool` file, or of a
    `.pairs` / `.pairs.gz` file's table in table order), or the Error: line to print when they cannot be paired (reference
    mustache.py:1019-1045, diff_mustache.py:781-800)."""
    if not ch or ch == 'n':
        from .pairs import is_pairs
        if not is_pairs(f) and not f.endswith((".cool", ".mcool", ".hic")):
            return "Error: Please enter the chromosome name."
        ch = _all_chromosomes(f, res, pairs_zero_based)
        if isinstance(ch, str):
            return ch
    ch2 = ch2 if isinstance(ch2, list) else ch
    if len(ch) != len(ch2):
        return "Error: the same number of chromosome1 and chromosome2 should be provided."
    return list(zip(ch, ch2))


def trans_all_pairs(f, res, ch, ch2, pairs_trans=False, pairs_zero_based=False):
    """--trans-all -> every unordered pair (A, B) of the -ch list in list order (without -ch: of every chromosome of `f`, in the
    file's order), or the Error: line of a run that `f` or -ch2 rules out."""
    why = (TRANS_ALL_CH2 if isinstance(ch2, list) else None) or trans_input([f], pairs_trans)
    if why:
        return "Error: %s" % why
    if not ch or ch == 'n':
        ch = _all_chromosomes(f, res, pairs_zero_based)
        if isinstance(ch, str):
            return ch
    ch = list(ch)
    return [(ch[i], ch[j]) for i in range(len(ch)) for j in range(i + 1, len(ch))]


# ----------------------------------------------------------------------------------------------------------------------
# the plan
# ----------------------------------------------------------------------------------------------------------------------
def plan(rq, res):
    """The Plan of the run `rq` asks for at resolution `res` (bp; false: -r could not be parsed), or the line to print when it
    cannot go ahead (refuse()).  Touches no GPU.  The order of the rules is DESIGN.md's "The order of refusals"."""
    files = rq.files
    if not all(f and os.path.exists(f) for f in files):
        return "Error: Couldn't find the specified contact files"
    if not res:
        return "Error: Invalid resolution"
    why = pairs_input(rq) or thinning_genome(rq) or thinning(rq) or multires_genome(rq, res) or multires(rq, res) \
        or (rq.pairs_trans and keep_trans_rows(files, rq.pairs_zero_based))
    if why:
        return "Error: %s" % why
    balance = None
    if rq.trans_all:
        why = (TRANS_ALL_CH2 if isinstance(rq.ch2, list) else None) or trans_input(files, rq.pairs_trans) \
            or balance_on_trans(rq.balance) or trans_ranks(rq.ranks)
        if why:
            return "Error: %s" % why
        cis, trans = [], trans_all_pairs(files[0], res, rq.ch, rq.ch2, rq.pairs_trans, rq.pairs_zero_based)
        if isinstance(trans, str):
            return trans
    else:
        pairs = chromosome_pairs(files[0], res, rq.ch, rq.ch2, rq.pairs_zero_based)
        if isinstance(pairs, str):
            return pairs
        for path, missing in rq.bias:
            if path and not os.path.exists(path):
                return "Error: %s" % missing
        why = None
        if rq.balance is not None:
            try:
                balance = check_request(rq.balance, files, given_bias(rq), rq.norm_method, rq.ranks, bias_flag=rq.bias_flag)
            except BalanceError as e:
                why = str(e)
        # inter-chromosomal pairs run after every intra-chromosomal pair, in pair order
        cis, trans = [p for p in pairs if p[0] == p[1]], [p for p in pairs if p[0] != p[1]]
        if trans and not why:
            why = (None if rq.ch and rq.ch != 'n' else NEED_CH) or balance_on_trans(rq.balance) or trans_ranks(rq.ranks)
        if why:
            return "Error: %s" % why
    genome = None
    if rq.balance_genome is not None or rq.balance_pixels_given:
        from .balance_genome import check_genome_request
        try:
            genome = check_genome_request(rq.balance_genome, rq.balance_pixels, files, given_bias(rq), rq.norm_method, rq.balance,
                                          rq.ranks, "none" if not trans else "some" if cis else "all", pairs_trans=rq.pairs_trans)
        except BalanceError as e:
            return "Error: %s" % e
    elif trans and not rq.trans_all and trans_input(files, rq.pairs_trans):
        return Raises(TEXT_ON_TRANS) if rq.text_pair_raises else "Error: %s" % TEXT_ON_TRANS
    return Plan(cis, trans, rq.trans_all, balance, genome)
