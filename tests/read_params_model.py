"""A plain model of read-parameter files (-r): the rows (BamController::load_read_params restating ReadMapParamsParser::init and
ReadParameters::parse_from_string / check_quality) and how they are served to the records of a BAM stream (BamController::serve_read_params
restating ReadMapParamsParser::get_read_params: a dict that is popped).  Written from the rules, byte strings throughout."""

OK, SKIP, CANT_PARSE_NO_COUNT, CANT_PARSE, LOW_QUALITY = range(5)
NONE = 0xFFFFFFFF


def split_lines(text):
    """The lines of one file's inflated bytes with their '\\n' (the last one may have none) and where each begins."""
    lines, offs, at = [], [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        end = len(text) if nl < 0 else nl + 1
        lines.append(text[at:end]); offs.append(at)
        at = end
    return lines, offs


def parse_row(line, min_phred):
    """None for an empty line; "malformed" for a line that gives no row; else dict(name, cb, umi, quality, ok)."""
    if line.endswith(b"\n"):              # (a '\r' goes only with the '\n' behind it)
        line = line[:-1]
        if line.endswith(b"\r"):
            line = line[:-1]
    if not line:
        return None
    parts, start = [], 0
    for _ in range(4):
        end = line.find(b" ", start)
        if end < 0:
            return "malformed"
        parts.append(line[start:end]); start = end + 1
    parts.append(line[start:])
    name, cb, umi, cbq, umiq = parts
    if name[:1] == b"@":
        name = name[1:]
    if not cb or not umi:
        return "malformed"
    ok = True
    if min_phred > 33:
        threshold = min_phred if min_phred < 128 else min_phred - 256      # char(min_phred), signed
        for q in cbq + umiq:
            ok = ok and (q if q < 128 else q - 256) >= threshold
    return dict(name=name, cb=cb, umi=umi, quality=umiq, ok=ok)


def pack(seq):
    """The 2-bit code of a barcode / UMI, 0 when it does not pack (empty, more than 31 bases, a letter outside ACGT)."""
    if not seq or len(seq) > 31:
        return 0
    c = 1
    for ch in seq:
        k = b"ACGT".find(bytes([ch]))
        if k < 0:
            return 0
        c = (c << 2) | k
    return c


class Rows:
    """Every line of the files in order (texts: one bytes object per file or per call), and the table: name -> first row."""

    def __init__(self, texts, min_phred):
        self.rows = []                     # per line: None / "malformed" / dict (+ 'canonical')
        self.first = {}
        min_phreds = min_phred if isinstance(min_phred, (list, tuple)) else [min_phred] * len(texts)
        for text, mp in zip(texts, min_phreds):
            for line in split_lines(text)[0]:
                r = parse_row(line, mp)
                if isinstance(r, dict):
                    r["canonical"] = self.first.setdefault(r["name"], len(self.rows))
                self.rows.append(r)

    def counts(self):
        valid = [r for r in self.rows if isinstance(r, dict)]
        return dict(rows=len(self.rows), valid=len(valid), malformed=sum(1 for r in self.rows if r == "malformed"),
                    repeated=sum(1 for k, r in enumerate(self.rows) if isinstance(r, dict) and r["canonical"] != k))

    def lookup(self, name):
        if name[:1] == b"@":
            name = name[1:]
        return self.first.get(name, NONE)


class Server:
    """The rows being served: a name is popped by the first record that asks, for the server's life."""

    def __init__(self, rows):
        self.rows = rows
        self.left = dict(rows.first)

    def serve(self, status, name):
        """status: what the reader says of the record before its parameters are asked for (OK; SKIP; CANT_PARSE_NO_COUNT; CANT_PARSE for a
        -g record on a chromosome the annotation lacks).  -> (status, row served or NONE)."""
        if status in (SKIP, CANT_PARSE_NO_COUNT):
            return status, NONE
        if name[:1] == b"@":
            name = name[1:]
        row = self.left.pop(name, None)
        if row is None:
            return CANT_PARSE, NONE
        if not self.rows.rows[row]["ok"]:
            return LOW_QUALITY, row
        return status, row
