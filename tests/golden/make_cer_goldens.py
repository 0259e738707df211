#!/usr/bin/env python3
"""Record the reference's basic_normalize (utils/transcribe.py) on a fixed list of strings -> tests/golden/g10_cer.json.

    python tests/golden/make_cer_goldens.py REFERENCE_CHECKOUT      # or B2S_REFERENCE=... in the environment

Runs where a reference checkout is at hand; the fixture holds data only (input text, locale, output as code points) and the tests
read nothing else.  utils/transcribe.py imports `editdistance` and `requests` at module level; neither is used by basic_normalize,
so empty stand-in modules take their place.
"""
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))

# (text, locale).  Punctuation: one or more characters of every category the function drops (Pc _ and U+203F, Pd - and U+2014,
# Ps ( [ and U+300C, Pe ) ] and U+300D, Pi U+00AB U+201C, Pf U+00BB U+201D, Po ! , . ? U+3002 U+00BF); symbols of other categories
# ($ + ^ U+20AC, digits) stay.  The seven locales that drop spaces, and en-us / de-de / fr-fr that keep them.
CASES = [
    ("", "en-us"),
    ("", "zh-cn"),
    ("   ", "en-us"),
    ("Hello, World!", "en-us"),
    ("  leading and trailing  ", "en-us"),
    ("runs   of\t\twhite\n space\r\nhere", "en-us"),
    ("ALL UPPER CASE", "en-us"),
    ("snake_case and under‿tie", "en-us"),
    ("well-known — dashes – here", "en-us"),
    ("(round) [square] {curly} 「corner」", "en-us"),
    ("«guillemets» “quotes” ‘single’", "fr-fr"),
    ("¿Qué tal? ¡Bien!", "es-es"),
    ("it's 5 o'clock; cost: $3.50 + 2^3 = €9", "en-us"),
    ("punctuation only: !?.,;:", "en-us"),
    ("!?.,;:", "en-us"),
    (" - ", "en-us"),
    ("a , b", "en-us"),
    ("café naïve Ångström", "fr-fr"),
    ("Straße ÜBER größe", "de-de"),
    ("İstanbul İ", "tr-tr"),
    ("你好， 世界！", "zh"),
    ("你好， 世界！", "zh-cn"),
    ("你 好 。 ABC def", "zh-tw"),
    ("香港  「地鐵」", "zh-hk"),
    ("こんにちは、 世界。 ガギ", "ja-jp"),
    ("안녕하세요, 세계!", "ko-kr"),
    ("한 글  Hangul", "ko-kr"),
    ("สวัสดี ครับ", "th-th"),
    ("你好， 世界！", "en-us"),
    ("안녕 하세요", "en-us"),
    ("tab\tin a no-space locale 　ideographic", "ja-jp"),
    ("ZH locale in upper case keeps spaces", "ZH-CN"),
    ("ÀÉÎÕÜ precomposed upper", "pt-br"),
    ("é already decomposed", "fr-fr"),
    ("ǅ titlecase digraph Ǆ", "hr-hr"),
    ("ﬁne ligature Ω ohm", "en-us"),
    ("non breaking spaces", "en-us"),
    ("…ellipsis… and †dagger", "en-us"),
    ("emoji \U0001F600 stays, math ≠ stays", "en-us"),
    ("  。  你  ", "zh-cn"),
    ("MiXeD, 中文 and English. ", "zh-cn"),
    ("trailing punctuation then space . ", "en-us"),
]


def load_transcribe(ref):
    for name in ("editdistance", "requests"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("b2s_reference_transcribe", os.path.join(ref, "utils", "transcribe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("B2S_REFERENCE")
    if not ref:
        raise SystemExit(__doc__)
    mod = load_transcribe(ref)
    cases = [{"text": t, "locale": loc, "out": [ord(c) for c in mod.basic_normalize(t, loc)]} for t, loc in CASES]
    with open(os.path.join(HERE, "g10_cer.json"), "w", encoding="ascii") as f:
        json.dump({"what": "basic_normalize(text, locale) of the reference's utils/transcribe.py; out = code points",
                   "cases": cases}, f, ensure_ascii=True, indent=0)
    print("wrote %d cases" % len(cases))


if __name__ == "__main__":
    main()
