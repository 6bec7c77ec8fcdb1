// Driven by make_v8_fixtures.py and tools/oracle_regex_soak.py --engine v8, on the build machine only: never by a test.
// Splits text and classifies code points with V8's own regex engine, the engine that defines TKZ_PATTERN_O200K
// (tokenizer_ts/src/tikTokenizer.ts:100 -- `new RegExp(pattern, "gu")`, iterated with exec() from lastIndex 0, :200-201).
//
// usage: node v8_split.js <tokenizerBuilder.ts> info      one JSON line: process.versions and the SHA-256 of each pattern string
//        node v8_split.js <tokenizerBuilder.ts> classes   0x110000 bytes on stdout: the class code of every code point (tkz_unicode_classes' coding)
//        node v8_split.js <tokenizerBuilder.ts> split     per input line {"p": 1|2|3, "t": text}: one output line, the flat JSON list
//                                                         [index, length, index, length, ...] of the matches in UTF-16 units
// The three pattern strings are read out of the TypeScript source at run time (none is copied here): the declarations between
// `const REGEX_PATTERN_1` and the function that follows them are evaluated with their type annotations removed.
"use strict";
const fs = require("fs");
const crypto = require("crypto");
const readline = require("readline");

function patterns(tsPath) {
  const src = fs.readFileSync(tsPath, "utf8");
  const a = src.indexOf("const REGEX_PATTERN_1");
  const b = src.indexOf("function ", a);
  if (a < 0 || b < 0) throw new Error("pattern declarations not found in " + tsPath);
  const decl = src.slice(a, b).replace(/^(const \w+): string(\[\])? =/gm, "$1 =");
  const got = new Function(decl + "\nreturn [REGEX_PATTERN_1, REGEX_PATTERN_2, REGEX_PATTERN_3];")();
  if (got.length !== 3 || got.some(s => typeof s !== "string" || !s.length)) throw new Error("unexpected pattern declarations");
  return got;
}

const [tsPath, mode] = process.argv.slice(2);
const pats = patterns(tsPath);

if (mode === "info") {
  const v = process.versions;
  const sha = {};
  pats.forEach((s, i) => { sha[i + 1] = crypto.createHash("sha256").update(Buffer.from(s, "utf8")).digest("hex"); });
  console.log(JSON.stringify({ node: v.node, v8: v.v8, icu: v.icu, unicode: v.unicode, pattern_sha256: sha }));
} else if (mode === "classes") {
  // 0 other, 1 Lu, 2 Ll, 3 Lt, 4 Lm, 5 Lo, 6 M, 7 N, 8 = \s; the surrogates are 0
  const tests = [[/\p{Lu}/u, 1], [/\p{Ll}/u, 2], [/\p{Lt}/u, 3], [/\p{Lm}/u, 4], [/\p{Lo}/u, 5], [/\p{M}/u, 6], [/\p{N}/u, 7], [/\s/u, 8]];
  const out = Buffer.alloc(0x110000);
  for (let cp = 0; cp < 0x110000; cp++) {
    if (cp >= 0xD800 && cp < 0xE000) continue;
    const ch = String.fromCodePoint(cp);
    let cls = 0, hits = 0;
    for (const [re, code] of tests) if (re.test(ch)) { cls = code; hits++; }
    if (hits > 1) throw new Error("U+" + cp.toString(16) + " is in two classes");
    out[cp] = cls;
  }
  process.stdout.write(out);
} else if (mode === "split") {
  const res = pats.map(s => new RegExp(s, "gu"));
  const rl = readline.createInterface({ input: process.stdin, terminal: false });
  rl.on("line", line => {
    const { p, t } = JSON.parse(line);
    const re = res[p - 1];
    const out = [];
    let m;
    re.lastIndex = 0;
    while ((m = re.exec(t))) out.push(m.index, m[0].length);
    process.stdout.write(JSON.stringify(out) + "\n");
  });
} else {
  throw new Error("mode?");
}
