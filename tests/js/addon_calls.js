'use strict';
/* Behaviour pin of the N-API shim (csrc/ht_napi.cc) on the CPU: the shim linked against tests/js/abi_stub.cc (a recording stand-in for the
 * C ABI, see its header for the forced-failure values) is driven through one deterministic list of calls, and every call's outcome — the
 * thrown error's constructor name and full message, or a digest of the return value (type, length, content hash) — is written out
 * together with the stub's log lines for that call.  tests/golden/addon_calls.json holds the transcript of the shim before its argument
 * handling was consolidated (tests/golden/make_addon_calls_golden.py); tests/test_addon_calls_cpu.py requires the working tree's shim to
 * reproduce it.  The overflow cases at the end have a hand-written expectation instead: the recorded shim let them through.
 *
 *   HT_STUB_LOG=<log file> node addon_calls.js <addon.node> <out.json>
 */
const fs = require('fs');
const A = require(require('path').resolve(process.argv[2]));
const LOG = process.env.HT_STUB_LOG;
const W = 8, H = 6, FRAME = W * H * 4, FRAME64 = W * H * 8, MAGIC = 7777;

let logSeen = 0;
function newLogLines() {
  const s = fs.existsSync(LOG) ? fs.readFileSync(LOG, 'utf8') : '';
  const lines = s.slice(logSeen).split('\n').filter(function (l) { return l.length > 0; });
  logSeen = s.length;
  return lines;
}

function fnv(bytes) {
  let h = 2166136261;
  for (let i = 0; i < bytes.length; i++) h = Math.imul(h ^ bytes[i], 16777619) >>> 0;
  return ('0000000' + h.toString(16)).slice(-8);
}
const names = new Map(); /* handles (napi externals) -> the name they go by in the transcript */
function isExternal(v) { return require('util').types.isExternal(v); }
function digest(v) {
  if (v === undefined || v === null || typeof v === 'number' || typeof v === 'boolean' || typeof v === 'string') return typeof v + ':' + String(v);
  if (ArrayBuffer.isView(v)) return { type: v.constructor.name, length: v.length, hash: fnv(new Uint8Array(v.buffer, v.byteOffset, v.byteLength)) };
  if (isExternal(v)) return 'external';
  const o = {};
  Object.keys(v).forEach(function (k) { o[k] = digest(v[k]); });
  return { object: o };
}
function show(v) {
  if (names.has(v)) return names.get(v);
  if (v === undefined) return 'undefined';
  if (Buffer.isBuffer(v)) return 'Buffer(' + v.length + ')';
  if (ArrayBuffer.isView(v)) return v.constructor.name + (v.length <= 8 ? '[' + Array.from(v).join(',') + ']' : '(' + v.length + ')') + (v.byteOffset ? '@' + v.byteOffset : '');
  if (Array.isArray(v)) return '[' + v.map(show).join(', ') + ']';
  if (isExternal(v)) return 'external';
  if (v && typeof v === 'object') return '{' + Object.keys(v).map(function (k) { return k + ': ' + show(v[k]); }).join(', ') + '}';
  return typeof v === 'string' ? JSON.stringify(v) : String(v);
}

const transcript = [];
/* one entry: the call, what came of it, every byte array argument as the call left it (in-place outputs), the stub's lines */
async function rec(name, args, into) {
  const e = { call: name + '(' + args.map(show).join(', ') + ')' };
  let r;
  try {
    r = A[name].apply(null, args);
    if (r && typeof r.then === 'function') {
      try { e.resolved = digest(r = await r); } catch (err) { e.rejected = err.constructor.name; e.message = err.message; r = undefined; }
    } else e.returned = digest(r);
  } catch (err) { e.threw = err.constructor.name; e.message = err.message; r = undefined; }
  const after = args.filter(function (a) { return a instanceof Uint8Array; }).map(function (a) { return a.length + ':' + fnv(a); });
  if (after.length) e.bytes_after = after;
  e.log = newLogLines();
  (into || transcript).push(e);
  return r;
}

function rgba(n) { const a = new Uint8Array((n === undefined ? 2 : n) * FRAME); for (let i = 0; i < a.length; i++) a[i] = (i * 13 + 5) & 255; return a; }
function bytes(n) { const a = new Uint8Array(n); for (let i = 0; i < n; i++) a[i] = (i * 3 + 1) & 255; return a; }
function i32(n) { const a = new Int32Array(n); for (let i = 0; i < n; i++) a[i] = i + 1; return a; }
function f64(n) { const a = new Float64Array(n); for (let i = 0; i < n; i++) a[i] = i + 0.25; return a; }
const PAIRS = function () { return new Int32Array([0, 1, 1, 0]); };
const CASCADE = Buffer.from('HTCB-stub-cascade');

async function main() {
  newLogLines(); /* loading the module reads the ABI version */
  const ctx = await rec('createContext', [{ device: 0, interval: 4, cascade: CASCADE, hitCapacity: 100, queueCapacity: 200, options: 'fp_sparse=0' }]);
  names.set(ctx, 'ctx');
  const ctx2 = await rec('createContext', [{ cascade: new Uint8Array(CASCADE) }]);
  names.set(ctx2, 'ctx2');
  const dead = await rec('createContext', [{ cascade: CASCADE }]);
  names.set(dead, 'deadCtx');
  const bare = await rec('createContext', [{ cascade: CASCADE }]); /* never gets a geometry */
  names.set(bare, 'bareCtx');
  for (const a of [[], [undefined], ['x'], [7], [{}], [{ cascade: 5 }], [{ cascade: CASCADE, device: 'x', interval: {}, hitCapacity: null, queueCapacity: 'y', options: 5 }]]) await rec('createContext', a);
  await rec('setGeometry', [ctx, W, H, 4, new Int32Array([W, H, 4, 3])]);
  await rec('setGeometry', [ctx2, W, H, 4, null]);
  const dev = await rec('deviceAlloc', [ctx, 4 * FRAME]); /* 768 bytes: 4 RGBA frames, 2 binary64 frames */
  names.set(dev, 'dev');
  const dev2 = await rec('deviceAlloc', [ctx, 2 * FRAME]);
  names.set(dev2, 'dev2');
  const freed = await rec('deviceAlloc', [ctx, 64]);
  names.set(freed, 'freedDev');
  const devOfDead = await rec('deviceAlloc', [dead, 64]);
  names.set(devOfDead, 'devOfDeadCtx');
  await rec('deviceFree', [ctx2, freed]); /* the wrong context: refused, the handle stays valid */
  await rec('deviceFree', [ctx, freed]);
  await rec('deviceFree', [ctx, freed]);
  await rec('destroy', [dead]);
  await rec('destroy', [dead]);
  for (const a of [[], ['x'], [dev], [5]]) await rec('destroy', a);
  await rec('camshiftReserve', [ctx, 4]);

  /* every other export: [name, arguments of a full call, number of required arguments] */
  const rect = function () { return new Int32Array([1, 1, 4, 3]); };
  const specs = [
    ['setGeometry', function () { return [ctx, W, H, 4, new Int32Array([W, H, 4, 3])]; }, 4],
    ['detect', function () { return [ctx, rgba(), 2, W, H, 1]; }, 5],
    ['detectAsync', function () { return [ctx, rgba(), 2, W, H, 1]; }, 5],
    ['grayscale', function () { return [ctx, rgba(), 2, W, H]; }, 5],
    ['whitebalance', function () { return [ctx, rgba(), 2, W, H]; }, 5],
    ['camshiftReserve', function () { return [ctx, 4]; }, 2],
    ['camshiftInit', function () { return [ctx, rgba(), 2, W, H, 1, i32(8)]; }, 7],
    ['camshiftTrack', function () { return [ctx, rgba(), 2, W, H, 1, 1]; }, 7],
    ['info', function () { return [ctx]; }, 1],
    ['deviceCount', function () { return []; }, 0],
    ['allgatherBest', function () { return [[ctx, ctx2], [f64(12), f64(12)], 2]; }, 3],
    ['hostAlloc', function () { return [64]; }, 1],
    ['deviceAlloc', function () { return [ctx, 64]; }, 2],
    ['deviceUpload', function () { return [ctx, dev, 16, bytes(FRAME)]; }, 4],
    ['deviceDownload', function () { return [ctx, dev, 16, new Uint8Array(FRAME)]; }, 4],
    ['upload', function () { return [ctx, rgba(), 2, W, H]; }, 5],
    ['bindDevice', function () { return [ctx, dev, 8, 2, FRAME]; }, 5],
    ['uploadAsync', function () { return [ctx, rgba(), 2]; }, 3],
    ['swapFrames', function () { return [ctx]; }, 1],
    ['detectEnqueue', function () { return [ctx, 33]; }, 1],
    ['detectCollect', function () { return [ctx]; }, 1],
    ['collectBest', function () { return [ctx, 2, 33]; }, 1],
    ['detectWhitebalance', function () { return [ctx, 2]; }, 2],
    ['whitebalanceBound', function () { return [ctx, 2]; }, 2],
    ['camshiftInitBound', function () { return [ctx, 2, 1, i32(8)]; }, 4],
    ['camshiftTrackBound', function () { return [ctx, 2, 1, 0, false]; }, 4],
    ['camshiftTrackCollect', function () { return [ctx, 2]; }, 2],
    ['camshiftInitPairs', function () { return [ctx, PAIRS(), i32(8)]; }, 3],
    ['camshiftTrackPairs', function () { return [ctx, PAIRS(), 0, false]; }, 3],
    ['camshiftTrackSequence', function () { return [ctx, 1, 2, 0, dev, new Float64Array([0, 2 * FRAME]), FRAME, true, false]; }, 7],
    ['camshiftSequenceCollect', function () { return [ctx, 2, 3, true]; }, 3],
    ['camshiftBackProject', function () { return [ctx, 2, 1, A.BP_RGBA8]; }, 4],
    ['camshiftBackProjectDevice', function () { return [ctx, 2, 1, A.BP_RGBA8, dev, 8, FRAME + 4]; }, 7],
    ['camshiftBackProjectPairs', function () { return [ctx, PAIRS(), A.BP_F64]; }, 3],
    ['camshiftBackProjectPairsDevice', function () { return [ctx, PAIRS(), A.BP_F64, dev, 0, FRAME64]; }, 6],
    ['drawFrames', function () { return [ctx, rgba(), 2, W, H, rect()]; }, 5],
    ['drawFramesDevice', function () { return [ctx, dev, 4, 2, W, H, W * 4 + 4, H * (W * 4 + 4), rect(), dev2, 0, FRAME, true]; }, 12],
    ['framesBound', function () { return [ctx]; }, 1],
    ['framesEnqueued', function () { return [ctx]; }, 1],
    ['graphLaunches', function () { return [ctx]; }, 1],
  ];
  const wrongArray = function (a) { return a instanceof Float64Array ? new Float32Array(a.length) : a instanceof Int32Array ? new Uint32Array(a.length) : new Uint16Array(a.length); };
  for (const [name, mk, need] of specs) {
    const full = mk().length;
    await rec(name, mk());                                             /* a full call */
    for (let k = full - 1; k >= 0; k--) {                              /* optional arguments omitted one by one, then too few */
      if (k === need || k === need - 1 || k === 0 || (k > need && k < full)) await rec(name, mk().slice(0, k));
    }
    for (let i = 0; i < full; i++) {                                   /* each argument in turn of the wrong type */
      for (const wrong of ['x', {}]) { const a = mk(); a[i] = wrong; await rec(name, a); }
      if (ArrayBuffer.isView(mk()[i])) { const a = mk(); a[i] = wrongArray(a[i]); await rec(name, a); }
      if (Array.isArray(mk()[i])) { const a = mk(); a[i] = a[i].slice(1); await rec(name, a); }
    }
    const a0 = mk();
    if (a0[0] === ctx) {                                               /* a destroyed context, a device buffer for the context */
      for (const c of [dead, dev]) { const a = mk(); a[0] = c; await rec(name, a); }
    }
    for (let i = 1; i < full; i++) {
      if (a0[i] !== dev && a0[i] !== dev2) continue;                   /* a freed buffer, a context for the buffer, a dead context's buffer */
      for (const d of [freed, ctx, devOfDead]) { const a = mk(); a[i] = d; await rec(name, a); }
    }
  }
  /* the optional arguments at their other values; null where null is a value */
  await rec('setGeometry', [ctx, W, H, 4, null]);
  await rec('collectBest', [ctx, 2, -1]);
  await rec('collectBest', [ctx, 'x', 'y']);
  await rec('camshiftTrackBound', [ctx, 2, 1, 1, true]);
  await rec('camshiftTrackBound', [ctx, 2, 1, 1, 'x']);
  await rec('camshiftTrackPairs', [ctx, PAIRS(), 1, true]);
  await rec('camshiftTrackSequence', [ctx, 1, 2, 1, dev, new Float64Array([FRAME]), FRAME, false, true]);
  await rec('camshiftTrackSequence', [ctx, 1, 2, 1, dev, new Float64Array([0, FRAME, 2 * FRAME]), FRAME, true, true]);
  await rec('camshiftSequenceCollect', [ctx, 2, 3, false]);
  await rec('camshiftBackProject', [ctx, 2, 1, A.BP_F64]);
  await rec('camshiftBackProjectPairs', [ctx, PAIRS(), A.BP_RGBA8]);
  await rec('camshiftBackProjectDevice', [ctx, 2, 1, A.BP_F64, dev, 0, FRAME64]);
  await rec('camshiftBackProjectPairsDevice', [ctx, PAIRS(), A.BP_RGBA8, dev, 0, FRAME]);
  await rec('drawFrames', [ctx, rgba(), 2, W, H, null]);
  await rec('drawFramesDevice', [ctx, dev, 0, 2, W, H, 0, 0, null, null, 0, 0, false]);
  await rec('drawFramesDevice', [ctx, dev, 0, 2, W, H, 0, 0, undefined, undefined, 0, 0]);
  await rec('drawFramesDevice', [bare, dev, 0, 2, W, H, 0, 0, null, dev2, 0, 0]);
  await rec('detect', [ctx, Buffer.from(rgba()), 2, W, H]);
  await rec('detect', [ctx, new Uint8ClampedArray(2 * FRAME), 2, W, H, 'x']);
  await rec('upload', [ctx, new Int8Array(2 * FRAME), 2, W, H]);
  for (const name of ['camshiftBackProject', 'camshiftBackProjectDevice', 'camshiftBackProjectPairs', 'camshiftBackProjectPairsDevice']) { /* no geometry */
    const a = specs.find(function (s) { return s[0] === name; })[1](); a[0] = bare; await rec(name, a);
  }

  /* boundaries: the last accepted and the first rejected value */
  const vary = async function (name, i, values) {
    const mk = specs.find(function (s) { return s[0] === name; })[1];
    for (const v of values) { const a = mk(); a[i] = v; await rec(name, a); }
  };
  for (const [name, i] of [['detect', 2], ['detectAsync', 2], ['grayscale', 2], ['whitebalance', 2], ['camshiftInit', 2], ['camshiftTrack', 2], ['upload', 2], ['bindDevice', 3],
    ['uploadAsync', 2], ['detectWhitebalance', 1], ['whitebalanceBound', 1], ['camshiftInitBound', 1], ['camshiftTrackBound', 1], ['camshiftTrackCollect', 1],
    ['camshiftTrackSequence', 2], ['camshiftSequenceCollect', 1], ['camshiftSequenceCollect', 2], ['camshiftBackProject', 1], ['camshiftBackProjectDevice', 1], ['drawFrames', 2],
    ['drawFramesDevice', 3], ['allgatherBest', 2]]) await vary(name, i, [1, 0, -1]);
  for (const name of ['detect', 'detectAsync', 'grayscale', 'whitebalance', 'camshiftInit', 'camshiftTrack', 'upload', 'drawFrames']) {
    await vary(name, 1, [new Uint8Array(2 * FRAME - 1), new Uint8Array(2 * FRAME + 1)]);
    await vary(name, 3, [0, -1]);
    await vary(name, 4, [0, -1]);
  }
  await vary('uploadAsync', 1, [new Uint8Array(2 * FRAME - 1), new Uint8Array(0)]);
  await vary('camshiftInit', 6, [i32(7), i32(9)]);
  await vary('camshiftInitBound', 3, [i32(7), i32(9)]);
  await vary('camshiftInitPairs', 2, [i32(7), i32(9)]);
  for (const name of ['camshiftInitPairs', 'camshiftTrackPairs', 'camshiftBackProjectPairs', 'camshiftBackProjectPairsDevice']) await vary(name, 1, [new Int32Array([0, 1, 1]), new Int32Array([0, 1]), new Int32Array(0)]);
  await rec('camshiftTrackPairs', [ctx, new Int32Array((1 << 24) + 2), 0, false]);
  await vary('camshiftBackProject', 3, [1, 2, -1]);
  await vary('camshiftBackProjectDevice', 3, [2]);
  await vary('camshiftBackProjectPairs', 2, [2]);
  await vary('camshiftBackProjectPairsDevice', 2, [2]);
  await vary('allgatherBest', 1, [[f64(12), f64(11)], [f64(12)], []]);
  await rec('allgatherBest', [[ctx, ctx], [f64(12), f64(12)], 2]);
  await rec('allgatherBest', [[ctx, dead], [f64(12), f64(12)], 2]);
  await rec('allgatherBest', [[ctx, dev], [f64(12), f64(12)], 2]);
  await rec('allgatherBest', [[], [], 2]);
  await vary('setGeometry', 4, [new Int32Array([W, H, 4]), new Int32Array(0), undefined]);
  await vary('drawFrames', 5, [new Int32Array([1, 1, 4]), undefined]);
  await vary('drawFramesDevice', 8, [new Int32Array([1, 1, 4])]);
  await vary('deviceAlloc', 1, [1, 0, 0.5, 2.5e11 + 1e6, NaN]);
  await vary('hostAlloc', 0, [1, 0, NaN, 2e12]);
  /* device ranges: the last byte exactly at, and one past, the end of dev (768 bytes) and dev2 (384) */
  await vary('deviceUpload', 2, [3 * FRAME, 3 * FRAME + 1, -1, 2.5e11, 2.6e11]);
  await vary('deviceUpload', 3, [bytes(4 * FRAME - 16), bytes(4 * FRAME - 15), bytes(0)]);
  await vary('deviceDownload', 2, [3 * FRAME, 3 * FRAME + 1, 4 * FRAME + 1, -1, 2.6e11]);
  await vary('deviceDownload', 3, [new Uint8Array(4 * FRAME - 16), new Uint8Array(4 * FRAME - 15)]);
  await vary('bindDevice', 2, [2 * FRAME, 2 * FRAME + 1, 4 * FRAME, 4 * FRAME + 1, -1]);
  await vary('bindDevice', 4, [2 * FRAME - 4, 2 * FRAME - 3, 0, -1, 2.5e11, 2.6e11]);
  await rec('bindDevice', [ctx, dev, 4 * FRAME, 1, 0]);
  await rec('bindDevice', [ctx, dev, 0, 4, FRAME]);
  await rec('bindDevice', [ctx, dev, 0, 5, FRAME]);
  await vary('camshiftTrackSequence', 5, [new Float64Array([2 * FRAME]), new Float64Array([0, 2 * FRAME + 1]), new Float64Array([-1]), new Float64Array([NaN]), new Float64Array(0),
    new Float64Array([4 * FRAME + 1]), new Float64Array([2.6e11])]);
  await vary('camshiftTrackSequence', 6, [2 * FRAME, 2 * FRAME + 1, 0, -1]);
  for (const name of ['camshiftBackProjectDevice']) {
    await vary(name, 5, [2 * FRAME - 4, 2 * FRAME - 3, -1]);                 /* 2 frames, stride FRAME + 4: 388 bytes from the offset */
    await vary(name, 6, [0, FRAME - 1, FRAME, 3 * FRAME - 8, 3 * FRAME - 7, -1]);  /* offset 8 */
  }
  await rec('camshiftBackProjectDevice', [ctx, 2, 1, A.BP_RGBA8, dev, 2 * FRAME, 0]);
  await rec('camshiftBackProjectDevice', [ctx, 2, 1, A.BP_RGBA8, dev, 2 * FRAME + 1, 0]);
  await rec('camshiftBackProjectDevice', [ctx, 1, 1, A.BP_F64, dev, FRAME64, 2.5e11]);
  await rec('camshiftBackProjectDevice', [ctx, 1, 1, A.BP_F64, dev, FRAME64 + 1, 0]);
  await rec('camshiftBackProjectDevice', [ctx, 2, 1, A.BP_F64, dev, 0, FRAME64 - 1]);
  await rec('camshiftBackProjectDevice', [ctx, 3, 1, A.BP_F64, dev, 0, 0]);
  await vary('camshiftBackProjectPairsDevice', 4, [0, 1, -1]);                    /* 2 binary64 frames fill dev exactly */
  await vary('camshiftBackProjectPairsDevice', 5, [0, FRAME64 - 1, FRAME64 + 1]);
  await rec('camshiftBackProjectPairsDevice', [ctx, PAIRS(), A.BP_RGBA8, dev, 2 * FRAME, 0]);
  await rec('camshiftBackProjectPairsDevice', [ctx, PAIRS(), A.BP_RGBA8, dev, 2 * FRAME + 1, 0]);
  await rec('camshiftBackProjectPairsDevice', [ctx, PAIRS(), A.BP_RGBA8, dev, 0, FRAME - 1]);
  await rec('camshiftBackProjectPairsDevice', [ctx, PAIRS(), A.BP_RGBA8, dev, 0, 3 * FRAME]);
  await rec('camshiftBackProjectPairsDevice', [ctx, PAIRS(), A.BP_RGBA8, dev, 0, 3 * FRAME + 1]);
  const dfd = function (o) { const a = [ctx, dev, 0, 2, W, H, 0, 0, null, dev2, 0, 0, false]; Object.keys(o).forEach(function (k) { a[k] = o[k]; }); return a; };
  for (const o of [{ 2: 2 * FRAME }, { 2: 2 * FRAME + 1 }, { 2: 4 * FRAME + 1 }, { 7: 3 * FRAME }, { 7: 3 * FRAME + 1 }, { 6: 4 * W * 4 }, { 6: 4 * W * 4 + 1 }, { 6: 4 * FRAME }, { 3: 1, 6: 4 * FRAME / H },
    { 3: 1, 6: 4 * FRAME / H + 1 }, { 10: 1 }, { 11: FRAME }, { 11: FRAME + 1 }, { 3: 1, 10: FRAME }, { 3: 1, 10: FRAME + 1 }, { 3: 1, 10: 2 * FRAME + 1 }, { 3: 4, 9: null }, { 3: 5, 9: null },
    { 4: 0 }, { 5: 0 }, { 4: -1 }, { 2: -1 }, { 6: -1 }, { 7: -1 }, { 10: -1 }, { 11: -1 }, { 2: 2.6e11 }, { 4: 1 << 30, 5: 1 << 30 }, { 7: 2.5e11, 3: 2147483647 }]) await rec('drawFramesDevice', dfd(o));

  /* hostAlloc / hostFree */
  const pinned = await rec('hostAlloc', [2 * FRAME]);
  if (pinned) {
    names.set(pinned, 'pinned');
    pinned.set(rgba());
    await rec('uploadAsync', [ctx, pinned, 2]);
    await rec('hostFree', [pinned.subarray(4)]);
    await rec('hostFree', [pinned.subarray(0, 8)]);
    await rec('hostFree', [new Uint8Array(pinned.buffer)]);
    await rec('hostFree', [pinned]);
    await rec('hostFree', [pinned]);
  }
  for (const a of [[], ['x'], [new Uint8Array(8)], [new Uint8Array(0)], [new Float64Array(2)], [ctx], [5]]) await rec('hostFree', a);

  /* every failing C-ABI call: ht_camshift_reserve(ctx, MAGIC + k) makes the k-th following call on ctx fail (abi_stub.cc) */
  const failing = async function (k, name, args) { await rec('camshiftReserve', [ctx, MAGIC + k]); await rec(name, args); };
  const spec = function (name) { return specs.find(function (s) { return s[0] === name; })[1](); };
  await rec('createContext', [{ device: MAGIC, cascade: CASCADE }]);
  await rec('camshiftReserve', [ctx, MAGIC]);
  await rec('hostAlloc', [MAGIC]);
  for (const [name, ks] of [['setGeometry', [1]], ['detect', [1]], ['detectAsync', [1]], ['grayscale', [1]], ['whitebalance', [1, 2, 3]], ['camshiftInit', [1, 2, 3]], ['camshiftTrack', [1, 2, 3]],
    ['allgatherBest', [1]], ['deviceAlloc', [1]], ['deviceUpload', [1]], ['deviceDownload', [1]], ['upload', [1, 2]], ['bindDevice', [1]], ['uploadAsync', [1]], ['swapFrames', [1]],
    ['detectEnqueue', [1]], ['detectCollect', [1]], ['collectBest', [1]], ['detectWhitebalance', [1]], ['whitebalanceBound', [1]], ['camshiftInitBound', [1]], ['camshiftTrackBound', [1]],
    ['camshiftTrackCollect', [1]], ['camshiftInitPairs', [1]], ['camshiftTrackPairs', [1]], ['camshiftTrackSequence', [1]], ['camshiftSequenceCollect', [1]], ['camshiftBackProject', [1]],
    ['camshiftBackProjectDevice', [1]], ['camshiftBackProjectPairs', [1]], ['camshiftBackProjectPairsDevice', [1]], ['drawFrames', [1]], ['drawFramesDevice', [1, 2]]]) {
    for (const k of ks) await failing(k, name, spec(name));
  }
  await failing(1, 'collectBest', [ctx, 2]);
  await failing(1, 'deviceFree', [ctx, dev2]);
  await rec('detectEnqueue', [ctx, MAGIC]);
  await rec('detectCollect', [ctx]);
  await rec('detectEnqueue', [ctx]);
  await rec('detectCollect', [ctx]);

  /* the overflow cases: expectations written by hand.  Each must be refused with the entry point's own range message before any C-ABI call that acts. */
  const octx = A.createContext({ cascade: CASCADE });
  names.set(octx, 'ctx');
  A.setGeometry(octx, W, H, 4, null);
  const odev = A.deviceAlloc(octx, 4 * FRAME);
  names.set(odev, 'dev');
  newLogLines();
  const overflow = [];
  const seqMsg = 'camshiftTrackSequence: a call\'s frames lie outside the device buffer';
  for (const [name, args, message] of [
    ['bindDevice', [octx, odev, 0, Math.pow(2, 30), Math.pow(2, 34)], 'bindDevice(ctx, dev, byteOffset, n, frameStride): outside the device buffer'],
    ['camshiftTrackSequence', [octx, 0, Math.pow(2, 30), 0, odev, new Float64Array([0]), Math.pow(2, 34), false, false], seqMsg],
    ['camshiftTrackSequence', [octx, 0, 1, 0, odev, new Float64Array([1e30]), FRAME, false, false], seqMsg],
    ['camshiftBackProjectDevice', [octx, Math.pow(2, 30) + 1, 0, A.BP_RGBA8, odev, 0, Math.pow(2, 34)],
      'camshiftBackProjectDevice(ctx, n, first, kind, dev, byteOffset, stride): outside the device buffer'],
    /* a pair list holds at most 2^23 pairs (the shim refuses longer ones as malformed), so 2^30 + 1 pairs cannot be passed: the longest list it admits */
    ['camshiftBackProjectPairsDevice', [octx, new Int32Array(1 << 24), A.BP_RGBA8, odev, 0, Math.pow(2, 34)],
      'camshiftBackProjectPairsDevice(ctx, pairs, kind, dev, byteOffset, stride): outside the device buffer'],
  ]) {
    const e = await rec(name, args, overflow).then(function () { return overflow[overflow.length - 1]; });
    /* the back-projection forms need the frame size for the check: ht_plane, a lookup, is the one line they may leave */
    e.acted = e.log.filter(function (l) { return l.indexOf('ht_plane ') !== 0; });
    e.expected = { threw: 'RangeError', message: message, acted: [] };
    e.ok = e.threw === 'RangeError' && e.message === message && e.acted.length === 0;
  }
  fs.writeFileSync(process.argv[3], JSON.stringify({ transcript: transcript, overflow: overflow }, null, 1) + '\n');
}
main().catch(function (e) { console.error(e); process.exit(1); });
