"""Date patterns (DESIGN.md §3 rule 18) restated in plain Python, sharing nothing with the C++.

parse(pattern, text) is the value of a time text in whole seconds, or None for a malformed one.  A
hand-written matcher decides whether the text is well formed; a well-formed text then goes through
datetime.strptime and calendar.timegm with the pattern translated to strptime's directives.  What
strptime does not know is done by hand: `k` and `K`, fractions of more than 6 digits, years of other
than 4 digits, and the truncation toward zero before 1970.

Also here: render() writes an instant under a pattern (the tests' texts), mutate() spoils a text,
and lines()/messages() are lines_ref / messages_ref with this module's parse() plugged in for the
time (their own files are not edited: their time-format-1 hook is swapped for the call)."""
import calendar
import datetime

NUMERIC = "yMdDHkhKmsS"
NATURAL = {"y": 4, "M": 2, "d": 2, "D": 3, "H": 2, "k": 2, "h": 2, "K": 2, "m": 2, "s": 2}
SHORT = ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]
FULL = ["January", "February", "March", "April", "May", "June", "July", "August", "September", "October",
        "November", "December"]
DIRECTIVE = {"M": "%m", "d": "%d", "D": "%j", "H": "%H", "k": "%H", "K": "%H", "h": "%I", "a": "%p", "m": "%M", "s": "%S",
             "S": "%f"}


def tokens(pattern):
    """[("lit", char) | (letter, count)]: quotes resolved, runs of one letter joined."""
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == "'":
            if pattern[i + 1:i + 2] == "'":
                out.append(("lit", "'"))
                i += 2
                continue
            i += 1
            while pattern[i] != "'" or pattern[i + 1:i + 2] == "'":
                if pattern[i] == "'":
                    i += 1
                out.append(("lit", pattern[i]))
                i += 1
            i += 1
        elif c.isalpha() and c.isascii():
            n = 1
            while pattern[i + n:i + n + 1] == c:
                n += 1
            out.append((c, n))
            i += n
        else:
            out.append(("lit", c))
            i += 1
    return out


def _numeric(tok):
    return tok[0] != "lit" and tok[0] in NUMERIC and not (tok[0] == "M" and tok[1] > 2)


def _widths(toks, k):
    """(least, most) digits of the numeric field toks[k]."""
    letter, n = toks[k]
    if letter == "y" and n == 2:
        return 2, 2
    if k + 1 < len(toks) and _numeric(toks[k + 1]):
        return n, n
    if letter == "S":
        return 1, n
    return 1, max(n, NATURAL[letter])


def _leap(y):
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def _month_len(y, m):
    return [31, 29 if _leap(y) else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31][m - 1]


def split(pattern, text):
    """The matcher: the text of every field, by letter, or None when the text does not fit the
    pattern's shape or a field is out of its range."""
    toks = tokens(pattern)
    got, i = {}, 0
    for k, (letter, n) in enumerate(toks):
        if letter == "lit":
            if text[i:i + 1] != n:
                return None
            i += 1
        elif _numeric((letter, n)):
            least, most = _widths(toks, k)
            j = i
            while j < len(text) and j - i < most and text[j] in "0123456789":
                j += 1
            if j - i < least:
                return None
            got[letter if not (letter == "y" and n == 2) else "yy"] = text[i:j]
            i = j
        elif letter == "M":
            names = SHORT if n == 3 else FULL
            hit = [m for m in names if text[i:i + len(m)].lower() == m.lower()]
            if not hit:
                return None
            name = max(hit, key=len)
            got["name"] = text[i:i + len(name)]
            got["month_of_name"] = names.index(name) + 1
            i += len(name)
        elif letter == "a":
            if text[i:i + 2].lower() not in ("am", "pm"):
                return None
            got["a"] = text[i:i + 2]
            i += 2
        elif letter == "Z":
            if text[i:i + 1] == "Z":
                got["Z"] = "Z"
                i += 1
                continue
            w = 6 if n == 2 else 5
            z = text[i:i + w]
            digits = z[1:3] + (z[4:6] if n == 2 else z[3:5])
            if len(z) != w or z[0] not in "+-" or not (digits.isdigit() and digits.isascii()) or (n == 2 and z[3] != ":"):
                return None
            if int(digits[:2]) > 23 or int(digits[2:]) > 59:
                return None
            got["Z"] = z
            i += w
        else:
            raise ValueError("letter %r" % letter)
    if i != len(text):
        return None
    lo_hi = {"M": (1, 12), "d": (1, 31), "D": (1, 366), "H": (0, 23), "k": (1, 24), "h": (1, 12), "K": (0, 11), "m": (0, 59), "s": (0, 59)}
    for letter, (lo, hi) in lo_hi.items():
        if letter in got and not lo <= int(got[letter]) <= hi:
            return None
    year = int(got["y"]) if "y" in got else (lambda v: v + (1900 if v >= 69 else 2000))(int(got["yy"]))
    if "D" in got:
        if int(got["D"]) > (366 if _leap(year) else 365):
            return None
    else:
        month = int(got["M"]) if "M" in got else got["month_of_name"]
        if int(got["d"]) > _month_len(year, month):
            return None
    return got


def parse(pattern, text):
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    got = split(pattern, text)
    if got is None:
        return None
    # the same instant as a text strptime reads: the fields in a fixed order, by the translated directives
    toks = tokens(pattern)
    fmt, txt = [], []
    year_by_hand = None
    for letter, n in toks:
        if letter == "lit":
            continue
        if letter == "y":
            if n == 2:
                fmt.append("%y"); txt.append(got["yy"])
            elif len(got["y"]) == 4 and int(got["y"]) >= 1:
                fmt.append("%Y"); txt.append(got["y"])
            else:
                year_by_hand = int(got["y"])
        elif letter == "M" and n > 2:
            fmt.append("%b" if n == 3 else "%B"); txt.append(got["name"])
        elif letter == "k":
            fmt.append("%H"); txt.append(str(int(got["k"]) % 24))
        elif letter == "S":
            fmt.append("%f"); txt.append(got["S"][:6])
        elif letter == "Z":
            fmt.append("%z"); txt.append(got["Z"].replace(":", ""))
        else:
            fmt.append(DIRECTIVE[letter]); txt.append(got[letter])
    if year_by_hand is not None:   # strptime's %Y is four digits, its smallest year 1: a leap year stands in, or not
        fmt.append("%Y"); txt.append("2000" if _leap(year_by_hand) else "2001")
    dt = datetime.datetime.strptime(" ".join(txt), " ".join(fmt))
    hour = dt.hour
    if "K" in got and got["a"].lower() == "pm":
        hour += 12
    off = dt.utcoffset().total_seconds() if dt.utcoffset() is not None else 0
    secs = calendar.timegm((dt.year, dt.month, dt.day, hour, dt.minute, dt.second)) - int(off)
    if year_by_hand is not None:
        secs += (datetime.date(1, 1, 1).toordinal() + _days_before_year(year_by_hand) - datetime.date(dt.year, 1, 1).toordinal()) * 86400
    if secs < 0 and dt.microsecond // 1000 > 0:
        secs += 1   # Java's getMillis() / 1000l
    return secs


def _days_before_year(y):
    """Days from 0001-01-01 to y-01-01 in the proleptic Gregorian calendar (y may be 0)."""
    p = y - 1
    return p * 365 + p // 4 - p // 100 + p // 400


# ---------------------------------------------------------------- writing texts
def render(pattern, f, rng=None):
    """The instant f (dict: Y M D H m s ms off_min, and doy) under `pattern`.  With rng: minimal
    digits where the rule allows them, names in any case, 'Z' for a zero offset, at random."""
    toks = tokens(pattern)
    out = []
    for k, (letter, n) in enumerate(toks):
        if letter == "lit":
            out.append(n)
            continue
        if _numeric((letter, n)):
            if letter == "y":
                s = "%02d" % (f["Y"] % 100) if n == 2 else str(f["Y"]).zfill(n)
            elif letter == "S":
                s = ("%03d" % f["ms"] + "".join(str((f["ms"] * 7 + j) % 10) for j in range(6)))[:n]
                if rng and rng.random() < 0.2 and not (k + 1 < len(toks) and _numeric(toks[k + 1])):
                    s = s[:rng.randint(1, n)]
            else:
                v = {"M": f["M"], "d": f["D"], "D": f["doy"], "H": f["H"], "k": f["H"] or 24, "h": f["H"] % 12 or 12,
                     "K": f["H"] % 12, "m": f["m"], "s": f["s"]}[letter]
                least, most = _widths(toks, k)
                s = str(v).zfill(n)
                if rng and least < len(s) and rng.random() < 0.3:
                    s = str(v)
            out.append(s)
        elif letter == "M":
            s = (SHORT if n == 3 else FULL)[(f["M"] - 1) % 12]
            out.append(_any_case(s, rng))
        elif letter == "a":
            out.append(_any_case("PM" if f["H"] >= 12 else "AM", rng))
        elif letter == "Z":
            o = f["off_min"]
            if o == 0 and rng and rng.random() < 0.5:
                out.append("Z")
            else:
                out.append("%s%02d%s%02d" % ("-" if o < 0 else "+", abs(o) // 60, ":" if n == 2 else "", abs(o) % 60))
    return "".join(out)


def _any_case(s, rng):
    if not rng:
        return s
    return rng.choice([s, s, s.upper(), s.lower()])


def fields(y, mo, d, h=0, mi=0, s=0, ms=0, off_min=0):
    f = dict(Y=y, M=mo, D=d, H=h, m=mi, s=s, ms=ms, off_min=off_min)
    f["doy"] = sum(_month_len(y, k) for k in range(1, min(mo, 12))) + d
    return f


def for_pattern(pattern, f):
    """f with the year brought into 1969-2068 for a pattern that writes two digits of it."""
    if ("y", 2) in tokens(pattern):
        f = dict(f, Y=1969 + (f["Y"] - 1969) % 100)
        f["D"] = min(f["D"], _month_len(f["Y"], f["M"]))
        f["doy"] = sum(_month_len(f["Y"], k) for k in range(1, f["M"])) + f["D"]
    return f


MUTATIONS = ("digit dropped", "digit added", "wrong literal", "day 31 of a short month", "second 60", "month 13",
             "lower-case name", "trailing byte")


def mutate(pattern, f, kind, rng):
    """The instant f written under `pattern` and spoiled in the way `kind` names.  A pattern without
    the field a kind aims at gives the unspoiled text (it must then read as before)."""
    if kind == "day 31 of a short month":
        g = dict(f, M=rng.choice([2, 4, 6, 9, 11]), D=31)
        g["doy"] = 366 + (1 if _leap(f["Y"]) else 0)   # (for `D`: one day past the year's end)
        return render(pattern, g, rng)
    if kind == "second 60":
        return render(pattern, dict(f, s=60), rng)
    if kind == "month 13":
        g = dict(f, M=13)
        return render(pattern, g, rng)
    text = render(pattern, f, rng)
    if kind == "lower-case name":
        return text.lower()
    if kind == "trailing byte":
        return text + rng.choice("0Z x")
    digits = [i for i, c in enumerate(text) if c.isdigit()]
    if kind == "digit dropped":
        i = rng.choice(digits)
        return text[:i] + text[i + 1:]
    if kind == "digit added":
        i = rng.choice(digits)
        return text[:i] + rng.choice("0123456789") + text[i:]
    if kind == "wrong literal":
        other = [i for i, c in enumerate(text) if not c.isalnum()] or list(range(len(text)))
        i = rng.choice(other)
        return text[:i] + ("#" if text[i] != "#" else "%") + text[i + 1:]
    raise ValueError(kind)


# ---------------------------------------------------------------- lines and messages under a pattern
class _AsFormat1:
    """A line format whose time goes through the time-format-1 hook of lines_ref / messages_ref."""

    def __init__(self, fmt):
        self._fmt = fmt

    def __getattr__(self, name):
        return 1 if name == "time_format" else getattr(self._fmt, name)


class _AsMessageFormat1:
    def __init__(self, mf):
        self.kind, self.keys, self.line = mf.kind, mf.keys, _AsFormat1(mf.line)


def _hook(pattern):
    def civil(field):
        v = parse(pattern, field)
        if v is None:
            raise ValueError("malformed time (%s)" % pattern)
        return v
    return civil


def lines(chunks, fmt):
    """lines_ref.parse for a LineFormat with a time_pattern."""
    import lines_ref
    keep = lines_ref.civil_time
    lines_ref.civil_time = _hook(fmt.time_pattern)
    try:
        return lines_ref.parse(chunks, _AsFormat1(fmt))
    finally:
        lines_ref.civil_time = keep


def messages(chunks, mf, strict=False):
    """messages_ref.parse for a MessageFormat whose line has a time_pattern."""
    import lines_ref
    import messages_ref
    keep = lines_ref.civil_time, messages_ref.TIME1
    lines_ref.civil_time = _hook(mf.line.time_pattern)
    messages_ref.TIME1 = "malformed time (%s)" % mf.line.time_pattern
    try:
        return messages_ref.parse(chunks, _AsMessageFormat1(mf), strict)
    finally:
        lines_ref.civil_time, messages_ref.TIME1 = keep
