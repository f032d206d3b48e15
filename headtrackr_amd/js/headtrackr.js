'use strict';
/*
 * headtrackr.js (MI355X edition) — JavaScript host of the HIP detect / track hot path.
 *
 * Exposes the reference's per-frame API under the reference's names so that code written against
 * auduno/headtrackr's `headtrackr.ccv`, `headtrackr.cascade`, `headtrackr.camshift`, `headtrackr.facetrackr` and
 * `headtrackr.getWhitebalance` runs unchanged, with the pixel work done by libheadtrackr_hip.so through the N-API addon
 * (headtrackr_hip.node, C ABI in include/headtrackr_hip.h).  Reference citations are /root/reference/src/<file>:<line>.
 *
 *   ccv.grayscale(canvas)                               ccv.js:22-32     -> ht_grayscale_batch
 *   ccv.detect_objects(canvas,cascade,interval,min_nb)  ccv.js:109-333   -> ht_detect_batch (pyramid + cascade scan);
 *                                                                            seq construction + grouping stay in JS
 *   ccv.array_group(seq,gfunc)                          ccv.js:34-107    (host, O(n^2) on a few dozen rects)
 *   camshift.Tracker / Histogram / Moments / Rectangle / TrackObj          camshift.js:49-378 -> ht_camshift_*
 *   camshift.MultiTracker                               several trackers on one canvas, one device call per frame -> ht_camshift_*_pairs;
 *                                                       camshift.pairSchedule = 'cluster' (before the first tracker): G workgroups per pair on large canvases
 *                                                       getBackProjectionImg(i) / getBackProjectionImgs() / getPdf(i) -> ht_camshift_backproject_pairs
 *   facetrackr.Tracker / TrackObj                       facetrackr.js:37-255  (state machine WB -> VJ -> CS)
 *   getWhitebalance(canvas)                             whitebalance.js:5-30 -> ht_whitebalance_batch
 * plus batch entry points that the single-frame browser API has no room for:
 *   ccv.detect_objects_batch(frames, n, w, h, cascade, interval, min_neighbors, opts)  -> Promise<Array<Array<rect>>>
 *   new ccv.DeviceBatch(w, h, n, opts)   frames resident in HBM, detect batches pipelined over several contexts (enqueue /
 *                                        collect-best / re-enqueue), fused whitebalance, camshift call sequences — the JS form
 *                                        of the loop bench.py times; every C-ABI export has a JS name (INTEGRATION.md)
 *   hostAlloc(bytes)                     pinned host memory for frames that cross PCIe every call
 *   ccv.drawFrames(video, canvas[, rect])  the loop's video -> canvas drawImage (main.js:170) scaled on the device -> ht_draw_frames_device;
 *                                           video may be {width, height, format: 'nv12' | 'i420' | 'yuyv' | 'uyvy', matrix, data} -> ht_draw_frames_yuv_device
 *
 * "canvas" is anything with width, height and getContext('2d') -> {getImageData, putImageData, drawImage,
 * createImageData}; ./canvas.js provides one for Node.  Failure conventions are the reference's: empty arrays,
 * confidence -10000, width == height == 0 — plus exceptions only for misuse of the native layer (no GPU, bad cascade).
 */
const path = require('path');
const fs = require('fs');
const pack = require('./cascade_pack.js');

let native = null;
function addon() {
  if (!native) {
    try {
      native = require('./headtrackr_hip.node');
    } catch (e) {
      throw new Error('headtrackr_hip.node could not be loaded (' + e.message + '); build it with `python -m headtrackr_amd.build`. ' +
        'There is no JavaScript fallback for the detection / tracking kernels.');
    }
  }
  return native;
}

const headtrackr = {};
headtrackr.rev = 2; /* main.js:13 */

/* ---- cascade ---------------------------------------------------------------------------------------------------- */

let builtinCascade = null;
Object.defineProperty(headtrackr, 'cascade', { /* cascade.js:19: the trained face cascade, rebuilt from data/cascade.bin */
  enumerable: true,
  get: function () {
    if (!builtinCascade) builtinCascade = pack.unpackCascade(fs.readFileSync(path.join(__dirname, '..', 'data', 'cascade.bin')));
    return builtinCascade;
  }
});

/* one native context per (cascade object, interval, GPU); contexts own device memory, so they are cached */
const contexts = new WeakMap();
function contextFor(cascade, interval, device, options) { /* options: ht_config.options string of the context (part of the cache key), or nothing */
  if (device === undefined) device = headtrackr.device | 0;
  let perCascade = contexts.get(cascade);
  if (!perCascade) { perCascade = new Map(); contexts.set(cascade, perCascade); }
  const key = interval + '@' + device + (options ? '?' + options : '');
  let c = perCascade.get(key);
  if (!c) {
    const cfg = { cascade: pack.packCascade(cascade), interval: interval, device: device };
    if (options) cfg.options = options;
    c = { handle: addon().createContext(cfg), w: 0, h: 0, batch: 0, device: device };
    perCascade.set(key, c);
  }
  return c;
}
/* the two schedules of the (tracker, frame) pair calls: 'workgroup' = one workgroup per pair (no option), 'cluster' = option
 * cs_pairs_cluster=1: a few pairs on large frames get G workgroups each and tall rects a row-split initTracker.  Same results. */
function pairScheduleOptions(v, who) {
  if (v === undefined || v === 'workgroup') return '';
  if (v === 'cluster') return 'cs_pairs_cluster=1';
  throw new RangeError(who + ": pairSchedule is 'workgroup' or 'cluster'");
}
headtrackr.device = 0; /* HIP device ordinal used by the single-frame (drop-in) entry points */
headtrackr.deviceCount = function () { return addon().deviceCount(); }; /* GPUs the `devices` option of the batch entry points can name */

/* pyramid level sizes exactly as ccv.js:110-127 computes them (Math.pow / Math.floor in V8), handed to the native
 * side so that no libm difference can move a level boundary */
function levelDims(w, h, cascade, interval) {
  const scale = Math.pow(2, 1 / (interval + 1));
  const next = interval + 1;
  const upto = Math.floor(Math.log(Math.min(cascade.width, cascade.height)) / Math.log(scale));
  const n = upto + next * 2;
  const d = new Int32Array(2 * n);
  d[0] = w; d[1] = h;
  for (let i = 1; i <= interval; i++) {
    d[2 * i] = Math.floor(w / Math.pow(scale, i));
    d[2 * i + 1] = Math.floor(h / Math.pow(scale, i));
  }
  for (let i = next; i < n; i++) {
    d[2 * i] = Math.floor(d[2 * (i - next)] / 2);
    d[2 * i + 1] = Math.floor(d[2 * (i - next) + 1] / 2);
  }
  return d;
}

function ensureGeometry(c, w, h, batch, cascade, interval) {
  if (c.w !== w || c.h !== h || c.batch < batch) {
    addon().setGeometry(c.handle, w, h, batch, levelDims(w, h, cascade, interval));
    c.w = w; c.h = h; c.batch = batch;
    c.boundImg = null;
  }
}

/* One frame, several consumers: facetrackr.Tracker.track() reads its canvas once and the state machine may run more than one
 * device routine on that frame (VJ detection followed by camshift.initTracker, facetrackr.js:97-108).  The ImageData object is
 * uploaded once (ht_upload_frames) and stays bound; the *Bound addon entry points then work on it.  Every other entry point that
 * binds frames of its own drops the marker. */
function bindFrame(c, img, cascade, interval) {
  if (c.boundImg === img) return;
  ensureGeometry(c, img.width, img.height, 1, cascade, interval);
  addon().upload(c.handle, img.data, 1, img.width, img.height);
  c.boundImg = img;
}
/* The marker lives for ONE public call: a host canvas may hand out the same ImageData object again with refreshed pixels (zero-copy
 * video wrappers do), so object identity says nothing across calls — every public entry point that used bindFrame drops it on return. */
function unbindFrames() {
  const per = contexts.get(headtrackr.cascade);
  if (per) per.forEach(function (c) { c.boundImg = null; });
}
headtrackr.hostAlloc = function (bytes) { return addon().hostAlloc(bytes); }; /* Uint8Array over pinned host memory */
/* leave the process NOW: live contexts are destroyed, stdout / stderr flushed, then _exit(code) — no runtime teardown (see ht_napi.cc) */
headtrackr.exitNow = function (code) { addon().exitNow(code | 0); };
headtrackr.hostFree = function (arr) { addon().hostFree(arr); }; /* explicit: the addon's handles carry no GC finalizers (see ht_napi.cc) */

/* ---- ccv ------------------------------------------------------------------------------------------------------------ */

headtrackr.ccv = {};

headtrackr.ccv.grayscale = function (canvas) { /* ccv.js:22-32, in place, returns the canvas */
  const ctx = canvas.getContext('2d');
  const img = ctx.getImageData(0, 0, canvas.width, canvas.height);
  if (canvas.width > 0 && canvas.height > 0) {
    const c = contextFor(headtrackr.cascade, 5);
    addon().grayscale(c.handle, img.data, 1, canvas.width, canvas.height);
    c.boundImg = null;
  }
  ctx.putImageData(img, 0, 0);
  return canvas;
};

/* The loop's video -> canvas copy (main.js:170, 312) between two canvas-like objects, on the device: drawImage(video, 0, 0, canvas.width,
 * canvas.height), or with rect = [sx, sy, sw, sh] (wholly inside the video) the 9-argument form.  The video's pixels are uploaded, scaled
 * with the declared resampler (ht_draw_frames_device) and copied back into the canvas: the bytes canvas.js's drawImage writes.  With an
 * addon that lacks the calls the canvas's own drawImage does it. */
/* YUV sources: names -> the numbers of include/headtrackr_hip.h, and the packed layout every YUV call here uses.  4:2:0 (NV12 / I420): a
 * frame is Y (w h bytes), then UV (NV12) or U, V (I420), ceil(w/2) x ceil(h/2) chroma samples.  NV12's chroma plane has to start at an
 * even device address: a frame of odd width and odd height is placed `lead` = 1 byte into its buffer, frames `step` = bytes + 1 apart.
 * Packed 4:2:2 (YUYV / UYVY, what an uncompressed webcam or a capture card delivers): ONE plane of 4-byte macropixels, 4 ceil(w/2) h bytes
 * at 2 B/px; a frame is a multiple of 4 bytes and starts at a multiple of 4, so lead = 0 and step = bytes.  The draw calls take them
 * (drawFrames, DeviceBatch draw / drawList / drawListBound, with opts.prefilter too), and so do cropFeeds / alignFeeds (the library unpacks
 * such a feed's frame to RGBA first). */
/* Rotated and mirrored feeds: `orientation` = 0..7 on a drawFrames video or a DeviceBatch source.  k & 3 quarter turns clockwise bring the
 * stored frame upright, k >> 2 mirrors it horizontally after the turn; width, height and the bytes describe the frame AS STORED, the draw is
 * that of the oriented frame and rects are in ITS coordinates.  It travels in bits 8..10 of the format number the addon already passes
 * (HT_ORIENT of headtrackr_hip.h). */
function orientBits(orientation, who) {
  if (orientation === undefined || orientation === null) return 0;
  if (!(Number.isInteger(orientation) && orientation >= 0 && orientation <= 7)) throw new RangeError(who + ': orientation is an integer 0..7');
  return orientation << 8;
}
const YUV_FORMATS = { nv12: 0, i420: 1, yuyv: 4, uyvy: 5 }, YUV_MATRICES = { bt601: 0, bt709: 1, 'bt601-full': 2, 'bt709-full': 3 };
function yuvLayout(width, height, format, matrix, who) {
  const fmt = YUV_FORMATS[format], mat = YUV_MATRICES[matrix === undefined ? 'bt601' : matrix];
  if (fmt === undefined) throw new RangeError(who + ": format is 'nv12', 'i420', 'yuyv' or 'uyvy'");
  if (mat === undefined) throw new RangeError(who + ": matrix is 'bt601', 'bt709', 'bt601-full' or 'bt709-full'");
  if (!(width > 0 && height > 0)) throw new RangeError(who + ': width and height must be positive');
  if (fmt >= 4) { const packed = 4 * ((width + 1) >> 1) * height; return { fmt: fmt, mat: mat, bytes: packed, lead: 0, step: packed }; }
  const bytes = width * height + 2 * ((width + 1) >> 1) * ((height + 1) >> 1), lead = fmt === 0 ? (bytes & 1) : 0;
  return { fmt: fmt, mat: mat, bytes: bytes, lead: lead, step: bytes + lead };
}

headtrackr.ccv.drawFrames = function (video, canvas, rect) {
  const w = canvas.width, h = canvas.height, vw = video.width, vh = video.height, ctx2d = canvas.getContext('2d'), A = addon();
  const grow = function (c, key, bytes) { /* two device buffers per context, kept between calls */
    if (!c[key] || c[key + 'Bytes'] < bytes) {
      if (c[key]) A.deviceFree(c.handle, c[key]);
      c[key] = A.deviceAlloc(c.handle, bytes); c[key + 'Bytes'] = bytes;
    }
    return c[key];
  };
  if (video.format !== undefined && video.format !== 'rgba') {
    /* a video-like object {width, height, format: 'nv12' | 'i420' | 'yuyv' | 'uyvy', matrix, data: Uint8Array}: there is no host route — a canvas cannot
     * draw planes — so an addon without the call is an error */
    const L = yuvLayout(vw, vh, video.format, video.matrix, 'ccv.drawFrames'), orient = orientBits(video.orientation, 'ccv.drawFrames');
    if (typeof A.drawFramesYuvDevice !== 'function') throw new Error('ccv.drawFrames: this headtrackr_hip.node has no drawFramesYuvDevice (rebuild it)');
    if (!(video.data instanceof Uint8Array) || video.data.length < L.bytes) throw new RangeError('ccv.drawFrames: video.data is a Uint8Array of w*h + 2*ceil(w/2)*ceil(h/2) bytes (yuyv / uyvy: 4*ceil(w/2)*h)');
    if (!(w > 0 && h > 0)) return canvas;
    const c = contextFor(headtrackr.cascade, 5);
    ensureGeometry(c, w, h, 1, headtrackr.cascade, 5);
    const out = ctx2d.createImageData(w, h), dsrc = grow(c, 'drawSrc', L.lead + L.bytes), ddst = grow(c, 'drawDst', w * h * 4);
    A.deviceUpload(c.handle, dsrc, L.lead, video.data.subarray(0, L.bytes));
    A.drawFramesYuvDevice(c.handle, dsrc, L.lead, 1, vw, vh, L.fmt | orient, L.mat, 0, rect ? Int32Array.from(rect) : null, ddst, 0, 0, false);
    A.deviceDownload(c.handle, ddst, 0, out.data);
    ctx2d.putImageData(out, 0, 0);
    return canvas;
  }
  /* (the RGBA route has no format to carry an orientation: an oriented RGBA feed is a DeviceBatch source) */
  if (orientBits(video.orientation, 'ccv.drawFrames')) throw new RangeError("ccv.drawFrames: orientation needs a video with format 'nv12', 'i420', 'yuyv' or 'uyvy' (an RGBA feed: DeviceBatch opts.sources)");
  if (typeof A.drawFramesDevice !== 'function' || typeof A.deviceDownload !== 'function' || !(w > 0 && h > 0 && vw > 0 && vh > 0)) {
    if (rect) ctx2d.drawImage(video, rect[0], rect[1], rect[2], rect[3], 0, 0, w, h); else ctx2d.drawImage(video, 0, 0, w, h);
    return canvas;
  }
  const c = contextFor(headtrackr.cascade, 5);
  ensureGeometry(c, w, h, 1, headtrackr.cascade, 5);
  const src = video.getContext('2d').getImageData(0, 0, vw, vh), out = ctx2d.createImageData(w, h);
  const dsrc = grow(c, 'drawSrc', vw * vh * 4), ddst = grow(c, 'drawDst', w * h * 4);
  A.deviceUpload(c.handle, dsrc, 0, src.data);
  A.drawFramesDevice(c.handle, dsrc, 0, 1, vw, vh, 0, 0, rect ? Int32Array.from(rect) : null, ddst, 0, 0, false);
  A.deviceDownload(c.handle, ddst, 0, out.data); /* behind the draw on the context's stream; waits */
  ctx2d.putImageData(out, 0, 0);
  return canvas;
};

/* union-find grouping with rank + path compression; class numbers in first-seen order (ccv.js:34-107) */
headtrackr.ccv.array_group = function (seq, gfunc) {
  const n = seq.length;
  const parent = new Int32Array(n).fill(-1), rank = new Int32Array(n);
  const rootOf = function (i) { while (parent[i] !== -1) i = parent[i]; return i; };
  const compress = function (i, root) { while (parent[i] !== -1) { const t = i; i = parent[i]; parent[t] = root; } };
  for (let i = 0; i < n; i++) {
    if (!seq[i]) continue;
    let root = rootOf(i);
    for (let j = 0; j < n; j++) {
      if (i === j || !seq[j] || !gfunc(seq[i], seq[j])) continue;
      const root2 = rootOf(j);
      if (root2 === root) continue;
      if (rank[root] > rank[root2]) {
        parent[root2] = root;
      } else {
        parent[root] = root2;
        if (rank[root] === rank[root2]) rank[root2]++;
        root = root2;
      }
      compress(j, root);
      compress(i, root);
    }
  }
  const index = new Array(n);
  let cat = 0;
  for (let i = 0; i < n; i++) {
    let j = -1;
    if (seq[i]) {
      const r = rootOf(i);
      if (rank[r] >= 0) rank[r] = ~cat++;
      j = ~rank[r];
    }
    index[i] = j;
  }
  return { index: index, cat: cat };
};

/* raw hits (index form) -> the reference's `seq` (ccv.js:227-234), scale_x by repeated multiplication (ccv.js:244-245) */
function hitsToSeq(hits, from, to, cascade, interval) {
  const scale = Math.pow(2, 1 / (interval + 1));
  const s = [1];
  const seq = [];
  for (let k = from; k < to; k++) {
    const i = hits.scale[k], q = hits.q[k];
    while (s.length <= i) s.push(s[s.length - 1] * scale);
    seq.push({ x: (hits.x[k] * 4 + (q & 1) * 2) * s[i], y: (hits.y[k] * 4 + (q >> 1) * 2) * s[i],
      width: cascade.width * s[i], height: cascade.height * s[i], neighbor: 1, confidence: hits.sum[k] });
  }
  return seq;
}

/* ccv.js:249-332: grouping, per-class mean + 0.5, nested-rectangle filter */
function groupSeq(seq, min_neighbors) {
  if (!(min_neighbors > 0)) return seq;
  const result = headtrackr.ccv.array_group(seq, function (r1, r2) {
    const distance = Math.floor(r1.width * 0.25 + 0.5);
    return r2.x <= r1.x + distance && r2.x >= r1.x - distance && r2.y <= r1.y + distance && r2.y >= r1.y - distance &&
      r2.width <= Math.floor(r1.width * 1.5 + 0.5) && Math.floor(r2.width * 1.5 + 0.5) >= r1.width;
  });
  const comps = [];
  for (let i = 0; i <= result.cat; i++) comps.push({ neighbors: 0, x: 0, y: 0, width: 0, height: 0, confidence: 0 });
  for (let i = 0; i < seq.length; i++) {
    const r = seq[i], c = comps[result.index[i]];
    if (c.neighbors === 0) c.confidence = r.confidence;
    ++c.neighbors;
    c.x += r.x; c.y += r.y; c.width += r.width; c.height += r.height;
    c.confidence = Math.max(c.confidence, r.confidence);
  }
  const seq2 = [];
  for (let i = 0; i < result.cat; i++) {
    const c = comps[i], n = c.neighbors;
    if (n >= min_neighbors) {
      seq2.push({ x: (c.x * 2 + n) / (2 * n), y: (c.y * 2 + n) / (2 * n), width: (c.width * 2 + n) / (2 * n),
        height: (c.height * 2 + n) / (2 * n), neighbors: n, confidence: c.confidence });
    }
  }
  const out = [];
  for (let i = 0; i < seq2.length; i++) {
    const r1 = seq2[i];
    let keep = true;
    for (let j = 0; j < seq2.length && keep; j++) {
      const r2 = seq2[j], distance = Math.floor(r2.width * 0.25 + 0.5);
      if (i !== j && r1.x >= r2.x - distance && r1.y >= r2.y - distance && r1.x + r1.width <= r2.x + r2.width + distance &&
          r1.y + r1.height <= r2.y + r2.height + distance && (r2.neighbors > Math.max(3, r1.neighbors) || r1.neighbors < 3)) keep = false;
    }
    if (keep) out.push(r1);
  }
  return out;
}

headtrackr.ccv._group = groupSeq; /* exposed for tests */
headtrackr.ccv._hitsToSeq = hitsToSeq; /* likewise */

/* ccv.js:109: `canvas` is expected to be gray already (byte 0 of each pixel is what the detector reads) */
headtrackr.ccv.detect_objects = function (canvas, cascade, interval, min_neighbors) {
  const w = canvas.width, h = canvas.height;
  const img = canvas.getContext('2d').getImageData(0, 0, w, h);
  canvas.data = img.data; /* the reference hangs the pixels on the caller's canvas (ccv.js:115) */
  if (!(w > 0 && h > 0)) return [];
  const c = contextFor(cascade, interval);
  ensureGeometry(c, w, h, 1, cascade, interval);
  const hits = addon().detect(c.handle, img.data, 1, w, h, addon().INPUT_GRAY_IN_R);
  c.boundImg = null;
  return groupSeq(hitsToSeq(hits, 0, hits.sum.length, cascade, interval), min_neighbors);
};

/* fused colour path used by facetrackr: ccv.grayscale + ccv.detect_objects without the intermediate canvas copy */
headtrackr.ccv.detect_objects_rgba = function (rgba, w, h, cascade, interval, min_neighbors) {
  if (!(w > 0 && h > 0)) return [];
  const c = contextFor(cascade, interval);
  ensureGeometry(c, w, h, 1, cascade, interval);
  const hits = addon().detect(c.handle, rgba, 1, w, h, addon().INPUT_RGBA);
  c.boundImg = null;
  return groupSeq(hitsToSeq(hits, 0, hits.sum.length, cascade, interval), min_neighbors);
};

/* the same on an ImageData that bindFrame() has (or will have) put on the device: no second upload (facetrackr's VJ step) */
function detectBoundImg(img, cascade, interval, min_neighbors) {
  const c = contextFor(cascade, interval);
  bindFrame(c, img, cascade, interval);
  addon().detectEnqueue(c.handle, addon().INPUT_RGBA);
  const hits = addon().detectCollect(c.handle);
  return groupSeq(hitsToSeq(hits, 0, hits.sum.length, cascade, interval), min_neighbors);
}

/* contiguous block of frames owned by `rank` (sizes differ by at most one) — the sharding of BASELINE.json configs[3] */
function shardRange(total, rank, world) {
  const base = Math.floor(total / world), rem = total % world;
  const start = rank * base + Math.min(rank, rem);
  return [start, start + base + (rank < rem ? 1 : 0)];
}

/* facetrackr's choice among the grouped rects of one frame (facetrackr.js:157-165: strict '>', first maximum wins) */
function bestOf(rects) {
  let best;
  for (let i = 0; i < rects.length; i++) if (best === undefined || rects[i].confidence > best.confidence) best = rects[i];
  return best;
}

/* n RGBA frames (one Uint8Array of n*w*h*4 bytes) -> Promise of n result lists; runs on the libuv pool.
 * opts.devices = [0, 1, ...]: the frames are block-sharded over these GPUs (one native context and one pool job per GPU, all in
 * flight together); opts.gather: after the detection every GPU's best-face rect per frame (facetrackr.js:147-175) is
 * all-gathered over RCCL / xGMI so that every GPU holds the whole batch's bounding boxes; the gathered table comes back as
 * result.best = [{x, y, width, height, confidence, neighbors} | null per frame]. */
headtrackr.ccv.detect_objects_batch = function (frames, n, w, h, cascade, interval, min_neighbors, opts) {
  cascade = cascade || headtrackr.cascade;
  interval = interval === undefined ? 5 : interval;
  min_neighbors = min_neighbors === undefined ? 1 : min_neighbors;
  opts = opts || {};
  const devices = (opts.devices && opts.devices.length) ? opts.devices : [headtrackr.device | 0];
  const world = Math.min(devices.length, n);
  const fbytes = w * h * 4;
  const jobs = [];
  for (let r = 0; r < world; r++) {
    const span = shardRange(n, r, world), cnt = span[1] - span[0];
    const c = contextFor(cascade, interval, devices[r]);
    ensureGeometry(c, w, h, cnt, cascade, interval);
    c.boundImg = null;
    const view = frames.subarray(span[0] * fbytes, span[1] * fbytes);
    jobs.push(addon().detectAsync(c.handle, view, cnt, w, h, addon().INPUT_RGBA).then(function (hits) {
      const out = [];
      let k = 0;
      for (let f = 0; f < cnt; f++) {
        out.push(groupSeq(hitsToSeq(hits, k, k + hits.counts[f], cascade, interval), min_neighbors));
        k += hits.counts[f];
      }
      return { ctx: c, rects: out };
    }));
  }
  return Promise.all(jobs).then(function (parts) {
    let all = [];
    parts.forEach(function (p) { all = all.concat(p.rects); });
    if (opts.gather) {
      const per = Math.ceil(n / world);
      const recs = parts.map(function (p) {
        const a = new Float64Array(6 * per); /* padding rows stay zero */
        p.rects.forEach(function (rects, f) {
          const b = bestOf(rects);
          if (b) a.set([b.x, b.y, b.width, b.height, b.confidence, b.neighbors === undefined ? 1 : b.neighbors], 6 * f);
          else a[6 * f + 4] = -10000; /* facetrackr.js:239 */
        });
        return a;
      });
      const g = addon().allgatherBest(parts.map(function (p) { return p.ctx.handle; }), recs, per);
      const best = [];
      for (let r = 0; r < world; r++) {
        const span = shardRange(n, r, world);
        for (let f = 0; f < span[1] - span[0]; f++) {
          const o = 6 * (r * per + f);
          best.push(g[o + 5] > 0 ? { x: g[o], y: g[o + 1], width: g[o + 2], height: g[o + 3], confidence: g[o + 4], neighbors: g[o + 5] } : null);
        }
      }
      all.best = best;
    }
    return all;
  });
};

/* ---- device-resident batches: the pipelined path -------------------------------------------------------------------------
 * new ccv.DeviceBatch(w, h, n, {cascade, interval, device, depth, sets, trackers, grouping, handoff}):
 *   `sets` frame sets of n RGBA frames each live in ONE device buffer (HBM); `depth` native contexts (own HIP streams, own pyramid
 *   arenas) take detect batches in turn so that `depth` batches are in flight while the host groups the previous one
 *   (ht_detect_enqueue + ht_detect_collect_best_requeue: the C2 / C4 loop of bench.py, from JavaScript).
 *     upload(frames, set = 0)              host -> HBM once (frames: Uint8Array of n*w*h*4 bytes)
 *     detectBest(batches, min_neighbors, set, flags) -> {best: Float64Array(6 n) [x,y,width,height,confidence,neighbors] of the
 *                                           last batch, hits, batches}; neighbors 0 / confidence -10000 = no face (facetrackr.js:239)
 *     detect(min_neighbors, set)           -> Array<Array<rect>>: exactly ccv.detect_objects' result per frame (parity path)
 *     whitebalance(set)                    -> Float64Array(n): getWhitebalance per frame, fused into a detect batch's gray pass
 *     detectStep(set) (= detectStepEnqueue + detectStepFinish) / trackStep(set) / trackEnqueue(set) + trackCollect() / ingest(pinned) / swap()   K frame-synchronous live feeds, one time step per call (below)
 *     initTrackers(rects, set) / trackSequence(sets[], calcAngles, outAll) -> Float64Array(9 n [* calls]): n camshift streams,
 *                                           one track() per listed frame set, ONE host call (ht_camshift_track_sequence)
 *     backProjection(set, kind)            -> Uint8Array(4 n w h) ('rgba8', default: getBackProjectionImg().data per frame) or
 *                                           Float64Array(n w h) ('f64': getPdf()[x][y] at [y][x]) of the n frames of `set` (-1: whatever is
 *                                           bound, as after swap()) through the batch's trackers, computed on the device
 *                                           (ht_camshift_backproject); tracker state is untouched; throws before initTrackers / detectStep
 *   opts.source = {width, height, sets}: a second device buffer of `sets` SOURCE-size frame sets (n frames of width x height each) and the
 *   loop's video -> canvas drawImage (main.js:170) between the two buffers, on the device (ht_draw_frames_device):
 *     uploadSource(frames, sset = 0)       host -> HBM once (frames: Uint8Array of n*width*height*4 bytes)
 *   opts.sourceFormat = 'nv12' | 'i420' | 'yuyv' | 'uyvy' (+ opts.sourceMatrix = 'bt601' (default) | 'bt709' | 'bt601-full' | 'bt709-full'): the source sets
 *   hold YUV 4:2:0 frames, each packed Y, then UV or U, V (width*height + 2*ceil(width/2)*ceil(height/2) bytes): uploadSource, draw and
 *   drawBound then move and read 1.5 B/px, the colour conversion is fused into the draw (ht_draw_frames_yuv_device)
 *     draw(sset, set, rect)                source set `sset` scaled onto work set `set` (rect: Int32Array [x, y, width, height] inside a source
 *                                           frame, default the whole frame); enqueue only, except that with depth > 1 it waits — the other
 *                                           contexts read the work set on streams of their own
 *   opts.sources = [{width, height, format = 'rgba' | 'nv12' | 'i420' | 'yuyv' | 'uyvy', matrix, orientation = 0..7, sets = 1}, ...] (instead of opts.source): one entry per feed,
 *   every feed with its own device buffer, size and format; ONE launch draws them all (ht_draw_list_device)
 *     uploadSourceOf(i, frame, sset = 0)   feed i's packed frame host -> HBM
 *     drawList(sset, set, rects, opts)     every feed onto its frame of frame set `set`; rects: null, or a rect / null per feed;
 *                                           opts.prefilter = 1..8: each canvas pixel the mean of a block of the draw's samples (ht_draw_list_filtered_device)
 *     drawListBound(sset, rects, opts)     the same into context 0's own frame buffer (bound): follow with the step functions at set = -1
 *     drawFilterFactors(rects, opts)       -> Int32Array(2 n): the block Nx, Ny opts.prefilter gives each feed under rects
 *     drawBound(sset, rect)                the same into context 0's own frame buffer, which becomes its bound frames: follow with the step
 *                                           functions at set = -1
 *     backProjectionPairs(set, pairs, kind) -> the same per (tracker, frame) pair, pair order: ht_camshift_backproject_pairs
 *     cropPairs(set, pairs, opts) / cropFeeds(sset, streams, opts) / cropResult()   each tracker's box cut from its frame / from its feed's own
 *                                           frame and scaled to a patch, on the device (below: "Face crops")
 *     alignPairs(set, pairs, opts) / alignFeeds(sset, streams, opts) / alignResult()   the same for the box ROTATED by the tracker's angle: the
 *                                           face upright (below: "Angle-aligned face crops")
 *     initPairs / trackPairs / trackPairsEnqueue / detectStepFinish(min_neighbors, {feeds})   trackers and frames paired freely (below);
                                           opts.trackers = tracker slots to reserve (default n)
   opts.pairSchedule = 'cluster': the pair calls of a few pairs on large frames (1080p feeds) run G workgroups per pair and tall rects a
   row-split initTracker (context option cs_pairs_cluster=1); 'workgroup' (default): one workgroup per pair.  The same results.
   opts.grouping = 'device': detectBest, detect, detectStepFinish and whitebalance take the device route — grouping and best face run
   behind the scan on the GPU (ht_detect_best_enqueue / _collect), the host receives one record per frame; 'host' (default) keeps the
   host route.  The results are the same bytes.
   opts.handoff = 'device' (needs grouping: 'device'): the step from a detect step's best faces to camshift.initTracker (facetrackr.js:97-107:
   confidence > -10, floor the rect) runs on the GPU too (ht_camshift_init_best).  detectStepEnqueue(set, min_neighbors, sel) then also
   enqueues the trackers' initialisation from the device's records — every feed with the centre-half fallback, or the feeds of sel.feeds
   without one — so that track steps may be enqueued at once, without waiting for the best faces; detectStepFinish(min_neighbors, sel)
   collects the best faces whenever the host wants them and returns what the host hand-off returns.  ONE difference: the trackers are
   re-initialised at the ENQUEUE point in stream order, not at the finish — a track step enqueued between the two already follows the new
   face.  'host' (default): detectStepFinish initialises them, as before.
     destroy() */
headtrackr.ccv.DeviceBatch = function (w, h, n, opts) {
  opts = opts || {};
  const cascade = opts.cascade || headtrackr.cascade, interval = opts.interval === undefined ? 5 : opts.interval;
  const device = opts.device === undefined ? (headtrackr.device | 0) : opts.device;
  /* batches in flight: 2.  (The Python host gains 6 % from a third batch at 256 x 320x240; this loop, whose calls drain the pipeline every
   * `batches` batches, loses 12 %: 1.03 M frames/s at 2, 0.90 M at 3 with 48-batch calls — pass {depth: 3} for long calls.) */
  const depth = Math.max(1, opts.depth || 2), sets = Math.max(1, opts.sets || 1);
  const A = addon(), fbytes = w * h * 4, setBytes = n * fbytes;
  /* opts.grouping: where a batch's raw hits are grouped and each frame's best face is chosen — 'host' (default: ht_detect_collect_best's
   * worker threads) or 'device' (ht_detect_best_enqueue behind every detect batch: one 64-byte record per frame comes back).  The same
   * bytes either way. */
  const grouping = opts.grouping === undefined ? 'host' : opts.grouping;
  if (grouping !== 'host' && grouping !== 'device') throw new RangeError("DeviceBatch: opts.grouping is 'host' or 'device'");
  const onDevice = grouping === 'device';
  if (onDevice && (typeof A.detectBestEnqueue !== 'function' || typeof A.collectBestDevice !== 'function' || typeof A.detectGrouped !== 'function'))
    throw new Error("DeviceBatch: this headtrackr_hip.node has no detectBestEnqueue / collectBestDevice / detectGrouped (rebuild it) — needed for grouping: 'device'");
  /* opts.handoff: who decides, from a detect step's best faces, which trackers are initialised with which rect — 'host' (default:
   * detectStepFinish, after it has collected them) or 'device' (ht_camshift_init_best behind the grouping, enqueued by detectStepEnqueue) */
  const handoff = opts.handoff === undefined ? 'host' : opts.handoff;
  if (handoff !== 'host' && handoff !== 'device') throw new RangeError("DeviceBatch: opts.handoff is 'host' or 'device'");
  const handoffOnDevice = handoff === 'device';
  if (handoffOnDevice && !onDevice) throw new RangeError("DeviceBatch: handoff: 'device' needs grouping: 'device'");
  if (handoffOnDevice && (typeof A.camshiftInitBest !== 'function' || typeof A.camshiftInitBestResult !== 'function'))
    throw new Error("DeviceBatch: this headtrackr_hip.node has no camshiftInitBest / camshiftInitBestResult (rebuild it) — needed for handoff: 'device'");
  /* the two halves of a batch on either route; the device route's requeue re-issues its grouping inside the library */
  const enqueueBest = function (c, flags, min_neighbors) { A.detectEnqueue(c, flags); if (onDevice) A.detectBestEnqueue(c, min_neighbors, 0); };
  const collectBest = function (c, min_neighbors, requeue) { return onDevice ? A.collectBestDevice(c, requeue) : A.collectBest(c, min_neighbors, requeue); };
  /* opts.pairSchedule: how initPairs / trackPairs / detectStepFinish(.., {feeds}) schedule their pairs — 'workgroup' (default) or
   * 'cluster' (every context is created with options 'cs_pairs_cluster=1') */
  const pairSchedule = opts.pairSchedule === undefined ? 'workgroup' : opts.pairSchedule;
  const ctxOptions = pairScheduleOptions(pairSchedule, 'DeviceBatch');
  const blob = pack.packCascade(cascade), dims = levelDims(w, h, cascade, interval);
  const ctxs = [];
  for (let i = 0; i < depth; i++) {
    const cfg = { cascade: blob, interval: interval, device: device };
    if (ctxOptions) cfg.options = ctxOptions;
    const hnd = A.createContext(cfg);
    A.setGeometry(hnd, w, h, n, dims);
    ctxs.push(hnd);
  }
  const dev = A.deviceAlloc(ctxs[0], sets * setBytes);
  const slots = Math.max(n, opts.trackers | 0); /* tracker slots reserved on first use: n, or opts.trackers when several trackers share a frame */
  let bound = -1, trackers = false;
  const pendingTrack = []; /* streams of the outstanding enqueue-only track steps, oldest first (pair steps need not have n) */
  const bind = function (set) { if (bound !== set) { ctxs.forEach(function (c) { A.bindDevice(c, dev, set * setBytes, n, fbytes); }); bound = set; } };
  this.width = w; this.height = h; this.frames = n; this.depth = depth; this.grouping = grouping; this.handoff = handoff; this.pairSchedule = pairSchedule;
  this.upload = function (frames, set) {
    if (frames.length < setBytes) throw new RangeError('DeviceBatch.upload: need n*w*h*4 bytes');
    A.deviceUpload(ctxs[0], dev, (set || 0) * setBytes, frames.subarray(0, setBytes));
  };
  this.detectBest = function (batches, min_neighbors, set, flags) {
    if (!(batches >= 1)) throw new RangeError('DeviceBatch.detectBest: batches must be >= 1');
    bind(set || 0);
    flags = flags === undefined ? A.INPUT_RGBA : flags;
    min_neighbors = min_neighbors === undefined ? 1 : min_neighbors;
    let started = Math.min(depth, batches), r = null;
    for (let i = 0; i < started; i++) enqueueBest(ctxs[i], flags, min_neighbors);
    for (let i = 0; i < batches; i++) { /* collect batch i; its context re-enqueues inside the call while batches remain */
      const more = started < batches;
      r = collectBest(ctxs[i % depth], min_neighbors, more ? flags : -1);
      if (more) started++;
    }
    r.batches = batches;
    return r;
  };
  this.detect = function (min_neighbors, set) {
    bind(set || 0);
    if (onDevice) { /* the frames' grouped lists are read from the device (ht_detect_grouped); min_neighbors 0: the seq list itself (ccv.js:232) */
      const mn = min_neighbors > 0 ? min_neighbors : 0, lists = [];
      enqueueBest(ctxs[0], A.INPUT_RGBA, mn);
      A.collectBestDevice(ctxs[0], -1);
      for (let f = 0; f < n; f++) {
        const g = A.detectGrouped(ctxs[0], f), list = [];
        for (let o = 0; o < g.length; o += 6) {
          list.push(mn > 0 ? { x: g[o], y: g[o + 1], width: g[o + 2], height: g[o + 3], neighbors: g[o + 5], confidence: g[o + 4] }
            : { x: g[o], y: g[o + 1], width: g[o + 2], height: g[o + 3], neighbor: 1, confidence: g[o + 4] });
        }
        lists.push(list);
      }
      return lists;
    }
    A.detectEnqueue(ctxs[0], A.INPUT_RGBA);
    const hits = A.detectCollect(ctxs[0]), out = [];
    let k = 0;
    for (let f = 0; f < n; f++) { out.push(groupSeq(hitsToSeq(hits, k, k + hits.counts[f], cascade, interval), min_neighbors)); k += hits.counts[f]; }
    return out;
  };
  this.whitebalance = function (set) {
    bind(set || 0);
    enqueueBest(ctxs[0], A.INPUT_RGBA | A.DETECT_WHITEBALANCE, 1);
    collectBest(ctxs[0], 1, -1);
    return A.detectWhitebalance(ctxs[0], n);
  };
  this.initTrackers = function (rects, set) { /* rects: Int32Array [x, y, width, height] per stream (camshift.js:198-211) */
    bind(set || 0);
    if (!trackers) { A.camshiftReserve(ctxs[0], slots); trackers = true; }
    A.camshiftInitBound(ctxs[0], n, 0, rects);
  };
  this.trackSequence = function (setList, calcAngles, outAll) {
    const offs = new Float64Array(setList.length);
    for (let k = 0; k < setList.length; k++) offs[k] = setList[k] * setBytes;
    return A.camshiftTrackSequence(ctxs[0], 0, n, calcAngles ? 1 : 0, dev, offs, fbytes, !!outAll, true);
  };
  /* K frame-synchronous feeds, one time step at a time (the K-feed form of the reference's loop, main.js:168-180 -> facetrackr.js:97-108,
   * 185-217): the n frames of `set` are the feeds' frames of this step.
   *   detectStep(set, min_neighbors) -> Float64Array(6 n) best face per feed (as detectBest) — and camshift.initTracker on its floor()ed
   *                                     rect (facetrackr.js:101-106); a feed without a face gets the centre half of the frame
   *   trackStep(set, calcAngles)     -> Float64Array(9 n): camshift.track per feed (enqueue-only launch + collect) */
  /*   ingest(pinned) / swap()        live ingest: the NEXT step's n frames cross PCIe from a hostAlloc() view on the copy stream while the
   *                                  current step is processed (ht_upload_frames_async / ht_swap_frames); after swap() pass set = -1 */
  const bind0 = function (set) { if (set >= 0) A.bindDevice(ctxs[0], dev, set * setBytes, n, fbytes); bound = -1; };
  this.ingest = function (pinned) { A.uploadAsync(ctxs[0], pinned, n); };
  this.swap = function () { A.swapFrames(ctxs[0]); bound = -1; };
  /*   detectStepEnqueue(set) / detectStepFinish(min_neighbors)   the two halves of detectStep: a streaming host enqueues the detect of
   *                                  step i right behind the track steps still in flight, collects THOSE (trackCollect), and only then
   *                                  waits for the best faces — the GPU does not idle while the host drains its pipeline */
  /*                                  (grouping 'device': detectStepEnqueue(set, min_neighbors) also enqueues the grouping, so that it runs
   *                                  behind the scan at once; detectStepFinish enqueues it itself when its min_neighbors differs) */
  /*                                  (handoff 'device': detectStepEnqueue(set, min_neighbors, sel) also enqueues initTracker from the device's
   *                                  best-face records — the trackers change HERE in stream order, and track steps may follow at once;
   *                                  detectStepFinish must be given the same min_neighbors and sel) */
  let stepGrouped = null; /* min_neighbors of the device grouping enqueued behind the step's detect, null: none yet */
  let stepHandoff = null; /* handoff 'device': {mn, feeds | null, pairs, fallback | null} of the initialisation the enqueue issued */
  const stepFeeds = function (what, sel) {
    if (!(sel && sel.feeds)) return null;
    const feeds = [];
    for (let i = 0; i < sel.feeds.length; i++) {
      const f = sel.feeds[i];
      if (!(f >= 0 && f < n)) throw new RangeError('DeviceBatch.' + what + ': feed ' + f + ' is not one of the ' + n + ' feeds');
      feeds.push(f);
    }
    return feeds;
  };
  this.detectStepEnqueue = function (set, min_neighbors, sel) {
    const feeds = handoffOnDevice ? stepFeeds('detectStepEnqueue', sel) : null; /* every check in front of the first enqueue */
    bind0(set === undefined ? 0 : set);
    A.detectEnqueue(ctxs[0], A.INPUT_RGBA);
    stepGrouped = null; stepHandoff = null;
    if (onDevice) { stepGrouped = min_neighbors === undefined ? 1 : min_neighbors; A.detectBestEnqueue(ctxs[0], stepGrouped, 0); }
    if (handoffOnDevice) {
      const list = feeds || Array.from({ length: n }, function (_v, f) { return f; });
      const pairs = new Int32Array(2 * list.length), fallback = feeds ? null : new Int32Array(4 * n);
      list.forEach(function (f, i) { pairs[2 * i] = f; pairs[2 * i + 1] = f; }); /* feed f's tracker is stream f, its frame is frame f of the batch */
      if (fallback) for (let f = 0; f < n; f++) fallback.set([w >> 2, h >> 2, w >> 1, h >> 1], 4 * f); /* no face: the centre half of the frame */
      if (list.length) { reserve(); A.camshiftInitBest(ctxs[0], pairs, -10, fallback); } /* facetrackr.js:97: confidence > -10 */
      stepHandoff = { mn: stepGrouped, feeds: feeds, pairs: pairs, fallback: fallback };
    }
  };
  this.detectStep = function (set, min_neighbors) {
    this.detectStepEnqueue(set, min_neighbors);
    return this.detectStepFinish(min_neighbors);
  };
  /* handoff 'device': the best faces, and what the enqueue's initialisation decided.  A pair whose record was not final on the device then
   * (a frame over the grouping cap) was deferred: its record is complete after the collect, and it is initialised now. */
  const finishOnDevice = function (mn, sel) {
    const ho = stepHandoff, feeds = stepFeeds('detectStepFinish', sel);
    if (!ho) throw new Error("DeviceBatch.detectStepFinish: no detectStepEnqueue outstanding (handoff: 'device')");
    const same = (feeds === null) === (ho.feeds === null) && (feeds === null || (feeds.length === ho.feeds.length && feeds.every(function (f, i) { return f === ho.feeds[i]; })));
    if (mn !== ho.mn || !same)
      throw new RangeError("DeviceBatch.detectStepFinish: min_neighbors and sel must be those of detectStepEnqueue (handoff: 'device': the trackers are already initialised)");
    stepGrouped = null; stepHandoff = null;
    const r = collectBest(ctxs[0], mn, -1), np = ho.pairs.length >> 1;
    let codes = new Int32Array(0), rects = new Int32Array(0);
    if (np) {
      const res = A.camshiftInitBestResult(ctxs[0], np);
      codes = res.codes; rects = res.rects;
      const late = [];
      for (let i = 0; i < np; i++) if (codes[i] === A.CSB_DEFERRED) late.push(i);
      if (late.length) {
        const lp = new Int32Array(2 * late.length), lf = ho.fallback ? new Int32Array(4 * late.length) : null;
        late.forEach(function (i, k) {
          lp[2 * k] = ho.pairs[2 * i]; lp[2 * k + 1] = ho.pairs[2 * i + 1];
          if (lf) lf.set(ho.fallback.subarray(4 * i, 4 * i + 4), 4 * k);
        });
        A.camshiftInitBest(ctxs[0], lp, -10, lf);
        const res2 = A.camshiftInitBestResult(ctxs[0], late.length);
        late.forEach(function (i, k) { codes[i] = res2.codes[k]; rects.set(res2.rects.subarray(4 * k, 4 * k + 4), 4 * i); });
      }
    }
    if (ho.feeds) {
      const found = [];
      for (let i = 0; i < np; i++) if (codes[i] === A.CSB_FACE) found.push(i);
      const rc = new Int32Array(4 * found.length);
      found.forEach(function (i, k) { rc.set(rects.subarray(4 * i, 4 * i + 4), 4 * k); });
      r.initialised = found.map(function (i) { return ho.feeds[i]; }); r.rects = rc;
      return r;
    }
    r.rects = new Int32Array(rects);
    return r;
  };
  this.detectStepFinish = function (min_neighbors, sel) {
    const mn = min_neighbors === undefined ? 1 : min_neighbors;
    if (handoffOnDevice) return finishOnDevice(mn, sel);
    if (onDevice && stepGrouped !== mn) A.detectBestEnqueue(ctxs[0], mn, 0);
    stepGrouped = null;
    const r = collectBest(ctxs[0], mn, -1);
    if (sel && sel.feeds) { /* feeds in different states: trackers only for the LISTED feeds that found a face (facetrackr.js:97) */
      const found = [];
      for (let i = 0; i < sel.feeds.length; i++) {
        const f = sel.feeds[i];
        if (!(f >= 0 && f < n)) throw new RangeError('DeviceBatch.detectStepFinish: feed ' + f + ' is not one of the ' + n + ' feeds');
        if (r.best[6 * f + 5] > 0 && r.best[6 * f + 4] > -10) found.push(f);
      }
      const pr = new Int32Array(2 * found.length), rc = new Int32Array(4 * found.length);
      found.forEach(function (f, i) {
        pr[2 * i] = f; pr[2 * i + 1] = f; /* feed f's tracker is stream f, its frame is frame f of the batch */
        for (let k = 0; k < 4; k++) rc[4 * i + k] = Math.floor(r.best[6 * f + k]);
      });
      if (found.length) { needPairs('detectStepFinish'); reserve(); A.camshiftInitPairs(ctxs[0], pr, rc); }
      r.initialised = found; r.rects = rc;
      return r;
    }
    const rects = new Int32Array(4 * n);
    for (let f = 0; f < n; f++) {
      const ok = r.best[6 * f + 5] > 0 && r.best[6 * f + 4] > -10;
      const v = ok ? [r.best[6 * f], r.best[6 * f + 1], r.best[6 * f + 2], r.best[6 * f + 3]] : [w >> 2, h >> 2, w >> 1, h >> 1];
      for (let k = 0; k < 4; k++) rects[4 * f + k] = Math.floor(v[k]);
    }
    if (!trackers) { A.camshiftReserve(ctxs[0], slots); trackers = true; }
    A.camshiftInitBound(ctxs[0], n, 0, rects);
    r.rects = rects;
    return r;
  };
  this.trackStep = function (set, calcAngles) {
    bind0(set === undefined ? 0 : set);
    A.camshiftTrackBound(ctxs[0], n, 0, calcAngles === false ? 0 : 1, false);
    return A.camshiftTrackCollect(ctxs[0], n);
  };
  /*   trackEnqueue(set, calcAngles) / trackCollect()   the two halves of trackStep: up to 4 track steps may be outstanding (the library
   *                                  keeps their results in a ring of pinned slots; trackCollect returns the OLDEST), so a streaming host
   *                                  enqueues step i + 1 before it waits for step i — the search window that links them lives on the GPU */
  this.trackEnqueue = function (set, calcAngles) {
    bind0(set === undefined ? 0 : set);
    A.camshiftTrackBound(ctxs[0], n, 0, calcAngles === false ? 0 : 1, false);
    pendingTrack.push(n);
  };
  this.trackCollect = function () { return A.camshiftTrackCollect(ctxs[0], pendingTrack.length ? pendingTrack.shift() : n); };
  /* Trackers and frames paired freely (ht_camshift_init_pairs / ht_camshift_track_pairs): pairs = Int32Array [stream, frame, ...] — any of
   * the opts.trackers slots (default n) in any order, each at most once per call, on any of the n frames of `set`, repeats allowed: several
   * faces of one frame each get a tracker, and of K feeds in different states (main.js:229-244) exactly those that track are tracked.  The
   * frame histogram is computed once per distinct frame.
   *   initPairs(set, pairs, rects)             camshift.initTracker per pair, rects: Int32Array [x, y, width, height] per pair
   *   trackPairs(set, pairs, calcAngles)       -> Float64Array(9 pairs), pair order
   *   trackPairsEnqueue(set, pairs, calcAngles) enqueue only; trackCollect() returns the oldest outstanding step, pair or not
   *   detectStepFinish(min_neighbors, {feeds}) best face of EVERY feed; trackers are initialised only for the listed feeds that found one
   *                                            (confidence > -10, facetrackr.js:97): result.initialised lists them, no centre-half substitute */
  const needPairs = function (what) {
    if (typeof A.camshiftInitPairs !== 'function' || typeof A.camshiftTrackPairs !== 'function')
      throw new Error('DeviceBatch.' + what + ': this headtrackr_hip.node has no camshiftInitPairs / camshiftTrackPairs (rebuild it)');
  };
  const reserve = function () { if (!trackers) { A.camshiftReserve(ctxs[0], slots); trackers = true; } };
  const pairList = function (what, pairs) {
    if (!(pairs instanceof Int32Array) || pairs.length < 2 || (pairs.length & 1)) throw new TypeError('DeviceBatch.' + what + ': pairs is an Int32Array [stream, frame, ...]');
    return pairs;
  };
  this.initPairs = function (set, pairs, rects) {
    needPairs('initPairs'); pairList('initPairs', pairs);
    if (!(rects instanceof Int32Array) || rects.length < 2 * pairs.length) throw new TypeError('DeviceBatch.initPairs: rects is an Int32Array [x, y, width, height] per pair');
    bind0(set === undefined ? 0 : set);
    reserve();
    A.camshiftInitPairs(ctxs[0], pairs, rects);
  };
  /* A tracker per grouped face, decided on the device (ht_camshift_init_faces; needs grouping: 'device'): the pairs naming one frame are,
   * in list order, that frame's slots (at most A.CSF_MAX_SLOTS), and the frame's grouped list of the device-grouped batch — the one
   * detectStepEnqueue(set, min_neighbors) put in flight, or the one detectStepFinish collected last — is dealt to them: faces with confidence >
   * minConfidence (default -10) by confidence rank, or with associate: true so that a tracker whose search window overlaps a face keeps its
   * slot.  The slot is the identity of a tracker across re-detections.  Enqueue only: track steps may follow at once.
   *   initFaces(pairs, {minConfidence, associate})
   *   initFacesResult() -> Int32Array(8 pairs): code (A.CSB_UNTOUCHED / CSB_FACE / CSB_DEFERRED), face (index in the frame's grouped list or
   *                        -1), x, y, width, height, dropped (eligible faces beyond the frame's slots), 0 per pair.  The slots of a frame
   *                        that was not final on the device (over the grouping cap) are deferred: once the batch has been collected
   *                        (detectStepFinish) initFacesResult() retries exactly those pairs, once, and returns the completed records
   *                        of the WHOLE pair list — then and at every later read, without another call to the device.
   * (camshift.MultiTracker.initFromDetection is not part of this: MultiTracker still initialises in list order from the host.) */
  let facesCall = null; /* {pairs, minConfidence, flags, merged} of the last initFaces; merged: its records once deferred pairs have been retried */
  const needFaces = function (what) {
    if (!onDevice) throw new RangeError('DeviceBatch.' + what + ": needs grouping: 'device'");
    if (typeof A.camshiftInitFaces !== 'function' || typeof A.camshiftInitFacesResult !== 'function')
      throw new Error('DeviceBatch.' + what + ': this headtrackr_hip.node has no camshiftInitFaces / camshiftInitFacesResult (rebuild it)');
  };
  this.initFaces = function (pairs, o) {
    needFaces('initFaces'); pairList('initFaces', pairs);
    o = o || {};
    const minConfidence = o.minConfidence === undefined ? -10 : o.minConfidence;
    if (typeof minConfidence !== 'number' || minConfidence !== minConfidence) throw new RangeError('DeviceBatch.initFaces: minConfidence is a number, not NaN');
    const flags = o.associate ? A.CSF_ASSOCIATE : 0;
    reserve();
    facesCall = null;
    A.camshiftInitFaces(ctxs[0], pairs, minConfidence, flags);
    facesCall = { pairs: new Int32Array(pairs), minConfidence: minConfidence, flags: flags, merged: null };
  };
  this.initFacesResult = function () {
    needFaces('initFacesResult');
    if (!facesCall) throw new Error('DeviceBatch.initFacesResult: no initFaces to report on');
    const fcall = facesCall, np = fcall.pairs.length >> 1;
    if (fcall.merged) return new Int32Array(fcall.merged); /* the library's last call is the retry now: its result names the late pairs only */
    const rec = A.camshiftInitFacesResult(ctxs[0], np);
    if (stepGrouped !== null) return rec; /* the batch is still in flight: deferred slots stay deferred until it has been collected */
    const late = [];
    for (let i = 0; i < np; i++) if (rec[8 * i] === A.CSB_DEFERRED) late.push(i);
    if (!late.length) return rec;
    const lp = new Int32Array(2 * late.length); /* every slot of a deferred frame is deferred: the frames keep their slots */
    late.forEach(function (i, k) { lp[2 * k] = fcall.pairs[2 * i]; lp[2 * k + 1] = fcall.pairs[2 * i + 1]; });
    A.camshiftInitFaces(ctxs[0], lp, fcall.minConfidence, fcall.flags);
    const rec2 = A.camshiftInitFacesResult(ctxs[0], late.length);
    const out = new Int32Array(rec);
    late.forEach(function (i, k) { out.set(rec2.subarray(8 * k, 8 * k + 8), 8 * i); });
    fcall.merged = out;
    return new Int32Array(out);
  };
  this.trackPairs = function (set, pairs, calcAngles) {
    needPairs('trackPairs'); pairList('trackPairs', pairs);
    bind0(set === undefined ? 0 : set);
    return A.camshiftTrackPairs(ctxs[0], pairs, calcAngles === false ? 0 : 1, true);
  };
  this.trackPairsEnqueue = function (set, pairs, calcAngles) {
    needPairs('trackPairsEnqueue'); pairList('trackPairsEnqueue', pairs);
    bind0(set === undefined ? 0 : set);
    A.camshiftTrackPairs(ctxs[0], pairs, calcAngles === false ? 0 : 1, false);
    pendingTrack.push(pairs.length >> 1);
  };
  this.backProjection = function (set, kind) {
    if (!trackers) throw new Error('DeviceBatch.backProjection: no trackers yet (initTrackers or detectStep first)');
    if (kind !== undefined && kind !== 'rgba8' && kind !== 'f64') throw new RangeError("DeviceBatch.backProjection: kind is 'rgba8' or 'f64'");
    bind0(set === undefined ? 0 : set);
    return A.camshiftBackProject(ctxs[0], n, 0, kind === 'f64' ? A.BP_F64 : A.BP_RGBA8);
  };
  /* output i: frame pairs[2i + 1] of `set` through the model of tracker pairs[2i] (ht_camshift_backproject_pairs) — the trackers of one
   * frame share its histogram and one pass over its pixels; the result is laid out like backProjection's, in pair order */
  this.backProjectionPairs = function (set, pairs, kind) {
    if (typeof A.camshiftBackProjectPairs !== 'function')
      throw new Error('DeviceBatch.backProjectionPairs: this headtrackr_hip.node has no camshiftBackProjectPairs (rebuild it)');
    pairList('backProjectionPairs', pairs);
    if (!trackers) throw new Error('DeviceBatch.backProjectionPairs: no trackers yet (initPairs, initTrackers or detectStep first)');
    if (kind !== undefined && kind !== 'rgba8' && kind !== 'f64') throw new RangeError("DeviceBatch.backProjectionPairs: kind is 'rgba8' or 'f64'");
    bind0(set === undefined ? 0 : set);
    return A.camshiftBackProjectPairs(ctxs[0], pairs, kind === 'f64' ? A.BP_F64 : A.BP_RGBA8);
  };
  const source = opts.source || null;
  /* opts.sourceFormat 'nv12' | 'i420' | 'yuyv' | 'uyvy' (+ opts.sourceMatrix): the source sets hold YUV frames at 1.5 B/px (4:2:0) or 2 B/px
   * (packed 4:2:2), packed as yuvLayout says */
  const yuv = source && opts.sourceFormat !== undefined && opts.sourceFormat !== 'rgba' ? yuvLayout(source.width, source.height, opts.sourceFormat, opts.sourceMatrix, 'DeviceBatch') : null;
  if (yuv && typeof A.drawFramesYuvDevice !== 'function') throw new Error('DeviceBatch: this headtrackr_hip.node has no drawFramesYuvDevice (rebuild it) — needed for opts.sourceFormat');
  const sframeBytes = source ? (yuv ? yuv.bytes : source.width * source.height * 4) : 0;
  const ssetBytes = source ? (yuv ? n * yuv.step + 2 * yuv.lead : n * sframeBytes) : 0; /* (a YUV set keeps the parity of its base) */
  const sdev = source ? A.deviceAlloc(ctxs[0], Math.max(1, source.sets || 1) * ssetBytes) : null;
  const needSource = function (what) { if (!sdev) throw new Error('DeviceBatch.' + what + ': created without opts.source'); };
  const ssetBase = function (sset) { return (sset || 0) * ssetBytes + (yuv ? yuv.lead : 0); };
  this.uploadSource = function (frames, sset) {
    needSource('uploadSource');
    if (frames.length < n * sframeBytes) throw new RangeError('DeviceBatch.uploadSource: need ' + (yuv ? 'n*(width*height + 2*ceil(width/2)*ceil(height/2))' : 'n*width*height*4') + ' bytes');
    if (!yuv || yuv.step === yuv.bytes) { A.deviceUpload(ctxs[0], sdev, ssetBase(sset), frames.subarray(0, n * sframeBytes)); return; }
    for (let f = 0; f < n; f++) A.deviceUpload(ctxs[0], sdev, ssetBase(sset) + f * yuv.step, frames.subarray(f * yuv.bytes, (f + 1) * yuv.bytes));
  };
  const drawSource = function (sset, rect, dst, doff, wait) {
    if (yuv) A.drawFramesYuvDevice(ctxs[0], sdev, ssetBase(sset), n, source.width, source.height, yuv.fmt, yuv.mat, yuv.step, rect || null, dst, doff, 0, wait);
    else A.drawFramesDevice(ctxs[0], sdev, ssetBase(sset), n, source.width, source.height, 0, 0, rect || null, dst, doff, 0, wait);
  };
  this.draw = function (sset, set, rect) {
    needSource('draw');
    drawSource(sset, rect, dev, (set || 0) * setBytes, depth > 1);
  };
  this.drawBound = function (sset, rect) {
    needSource('drawBound');
    drawSource(sset, rect, null, 0, false);
    bound = -1;
  };
  /* opts.sources = [{width, height, format = 'rgba' | 'nv12' | 'i420' | 'yuyv' | 'uyvy', matrix, orientation = 0 (orientBits), sets = 1}, ...]: one entry per feed, each feed with a device
   * buffer of its own that holds `sets` packed frames (RGBA rows; Y, then UV or U, V — an odd x odd NV12 frame one byte into its slot, as
   * yuvLayout says).  drawList / drawListBound draw all n feeds in ONE launch (ht_draw_list_device), every feed under a rect of its own. */
  const DRAW_RGBA = 16; /* HT_DRAW_RGBA */
  if (opts.sources !== undefined && opts.sources !== null && source) throw new Error('DeviceBatch: opts.sources together with opts.source (one or the other)');
  let feeds = null;
  if (opts.sources !== undefined && opts.sources !== null) {
    if (!Array.isArray(opts.sources) || opts.sources.length !== n) throw new RangeError('DeviceBatch: opts.sources is an array with one entry per feed (' + n + ')');
    if (typeof A.drawListDevice !== 'function') throw new Error('DeviceBatch: this headtrackr_hip.node has no drawListDevice (rebuild it) — needed for opts.sources');
    const layouts = opts.sources.map(function (s, i) {
      if (!s || typeof s !== 'object') throw new TypeError('DeviceBatch: opts.sources[' + i + '] is {width, height, format, matrix, sets}');
      if (!(Number.isInteger(s.width) && Number.isInteger(s.height) && s.width > 0 && s.height > 0)) throw new RangeError('DeviceBatch: opts.sources[' + i + ']: width and height must be positive integers');
      const sets = s.sets === undefined ? 1 : s.sets;
      if (!(Number.isInteger(sets) && sets >= 1)) throw new RangeError('DeviceBatch: opts.sources[' + i + ']: sets must be >= 1');
      const orient = orientBits(s.orientation, 'DeviceBatch: opts.sources[' + i + ']');
      if (s.format === undefined || s.format === 'rgba') return { width: s.width, height: s.height, fmt: DRAW_RGBA | orient, mat: 0, bytes: s.width * s.height * 4, lead: 0, step: s.width * s.height * 4, sets: sets };
      const L = yuvLayout(s.width, s.height, s.format, s.matrix, 'DeviceBatch: opts.sources[' + i + ']');
      return { width: s.width, height: s.height, fmt: L.fmt | orient, mat: L.mat, bytes: L.bytes, lead: L.lead, step: L.step, sets: sets };
    });
    feeds = layouts.map(function (f) { f.dev = A.deviceAlloc(ctxs[0], f.sets * f.step + 2 * f.lead); return f; });
  }
  const needFeeds = function (what) { if (!feeds) throw new Error('DeviceBatch.' + what + ': created without opts.sources'); };
  const feedBase = function (f, sset, what) {
    const k = sset === undefined ? 0 : sset;
    if (!(Number.isInteger(k) && k >= 0 && k < f.sets)) throw new RangeError('DeviceBatch.' + what + ': source set ' + sset + ' is not one of the feed\'s ' + f.sets);
    return k * f.step + f.lead;
  };
  this.uploadSourceOf = function (i, frame, sset) {
    needFeeds('uploadSourceOf');
    if (!(Number.isInteger(i) && i >= 0 && i < n)) throw new RangeError('DeviceBatch.uploadSourceOf: feed ' + i + ' is not one of the ' + n + ' feeds');
    const f = feeds[i];
    if (!frame || !(frame.length >= f.bytes)) throw new RangeError('DeviceBatch.uploadSourceOf: feed ' + i + ' needs ' + f.bytes + ' bytes');
    A.deviceUpload(ctxs[0], f.dev, feedBase(f, sset, 'uploadSourceOf'), frame.subarray(0, f.bytes));
  };
  const listEntries = function (sset, rects, what) {
    needFeeds(what);
    if (rects !== null && rects !== undefined && (!Array.isArray(rects) || rects.length !== n)) throw new TypeError('DeviceBatch.' + what + ': rects is null or an array with a rect or null per feed');
    return feeds.map(function (f, i) {
      let r = rects ? rects[i] : null;
      if (r !== null && r !== undefined) {
        const ok = (Array.isArray(r) || r instanceof Int32Array) && r.length === 4 && Array.prototype.every.call(r, Number.isInteger);
        if (!ok) throw new TypeError('DeviceBatch.' + what + ': rects[' + i + '] is [x, y, width, height] (integers) or null');
        r = Int32Array.from(r);
      }
      return { dev: f.dev, offset: feedBase(f, sset, what), width: f.width, height: f.height, format: f.fmt, matrix: f.mat, rect: r || null };
    });
  };
  /* opts.prefilter = 1..8 (ht_draw_list_filtered_device): every canvas pixel the mean of an Nx x Ny block of the unfiltered draw's samples, the
   * factors up to opts.prefilter per feed (drawFilterFactors gives them) — for strong downscales, where the plain draw reads 2 of every
   * ratio rows and columns.  Without it nothing changes.  The rect -> canvas mapping does not depend on the filter: cropFeeds' opts.rects
   * are the rects drawn, as before. */
  const drawPrefilter = function (what, o) {
    if (o !== undefined && o !== null && typeof o !== 'object') throw new TypeError('DeviceBatch.' + what + ': opts is an object ({prefilter})');
    return prefilterOf(what, o || {}, ['drawListFilteredDevice']);
  };
  this.drawList = function (sset, set, rects, o) {
    const mf = drawPrefilter('drawList', o), entries = listEntries(sset, rects, 'drawList');
    if (mf) A.drawListFilteredDevice(ctxs[0], entries, mf, dev, 0, (set || 0) * setBytes, depth > 1);
    else A.drawListDevice(ctxs[0], entries, dev, 0, (set || 0) * setBytes, depth > 1);
  };
  this.drawListBound = function (sset, rects, o) {
    const mf = drawPrefilter('drawListBound', o), entries = listEntries(sset, rects, 'drawListBound');
    if (mf) A.drawListFilteredDevice(ctxs[0], entries, mf, null, 0, 0, false);
    else A.drawListDevice(ctxs[0], entries, null, 0, 0, false);
    bound = -1;
  };
  /* Int32Array(2 n): Nx, Ny a draw of `rects` with opts.prefilter takes for each feed (the library's rule; no device work) */
  this.drawFilterFactors = function (rects, o) {
    const mf = prefilterOf('drawFilterFactors', o || {}, ['drawFilterFactors']);
    if (!mf) throw new RangeError('DeviceBatch.drawFilterFactors: opts.prefilter is an integer 1..8');
    const sizes = new Int32Array(2 * n);
    listEntries(0, rects, 'drawFilterFactors').forEach(function (e, i) {
      const odd = (e.format >> 8) & 1; /* an odd orientation: the whole source is height x width */
      sizes[2 * i] = e.rect ? e.rect[2] : (odd ? e.height : e.width); sizes[2 * i + 1] = e.rect ? e.rect[3] : (odd ? e.width : e.height);
    });
    return A.drawFilterFactors(sizes, w, h, mf);
  };
  /* Face crops on the device (ht_camshift_crop_pairs_device / ht_camshift_crop_sources_device): each tracker's box, as its last track step
   * — enqueue-only ones included — leaves it on the device, is cut from the frame and scaled to opts.width x opts.height RGBA.  Enqueue
   * only: nothing is fetched until cropResult().
   *   cropPairs(set, pairs, opts)      patch i: tracker pairs[2i] cut from frame pairs[2i + 1] of frame set `set` (-1: whatever is bound)
   *   cropFeeds(sset, streams, opts)   opts.sources batches: patch i: tracker streams[i] cut from feed i's OWN frame of source set `sset`;
   *                                    opts.rects = the rects that were drawn onto the canvas (drawList's rects; default the whole sources)
   *   cropResult()                     -> {n, width, height, records: Int32Array(6 n) [code, stream, x, y, width, height] (source pixels; code
   *                                    CROP_EMPTY: a lost or never tracked tracker, zeros), ratios: Float64Array(2 n), patches: Uint8Array(n width height 4)}
   *                                    of the LAST crop call; waits for it
   *   opts = {width, height (1..1024), margin = 1 (0.25..4: the box widened around its centre, in steps of 1/256), square = false} */
  /* Model-input tensors: with opts.tensor = {dtype: 'f32' | 'f16' | 'bf16', layout: 'chw' | 'hwc', channels: 'rgb' | 'bgr' | 'gray', scale, bias}
   * (scale, bias: a number for all channels or an array with one per output channel; defaults 1 / 255 and 0) the four calls write the
   * network's input instead of RGBA — every element fl32(fl32(byte * scale[c]) + bias[c]) rounded to the dtype, in the same single launch
   * (ht_camshift_*_tensor_device) — and cropResult() / alignResult() return `patches` as a Float32Array, or as a Uint16Array of the raw
   * f16 / bf16 bits, with `tensor: {dtype, layout, channels, shape}`.  An empty entry is bias[c] everywhere: read the record's code. */
  const TENSOR_DTYPES = { f32: 0, f16: 1, bf16: 2 }, TENSOR_LAYOUTS = { chw: 0, hwc: 1 }, TENSOR_CHANNELS = { rgb: 0, bgr: 1, gray: 2 };
  const tensorFormat = function (what, t, names) {
    if (t === undefined || t === null) return null;
    if (typeof t !== 'object') throw new TypeError('DeviceBatch.' + what + ': opts.tensor is {dtype, layout, channels, scale, bias}');
    if (names.some(function (f) { return typeof A[f] !== 'function'; }))
      throw new Error('DeviceBatch.' + what + ': this headtrackr_hip.node has no ' + names.join(' / ') + ' (rebuild it)');
    const dtype = t.dtype === undefined ? 'f16' : t.dtype, layout = t.layout === undefined ? 'chw' : t.layout, channels = t.channels === undefined ? 'rgb' : t.channels;
    if (!(dtype in TENSOR_DTYPES)) throw new RangeError('DeviceBatch.' + what + ": opts.tensor.dtype is 'f32', 'f16' or 'bf16'");
    if (!(layout in TENSOR_LAYOUTS)) throw new RangeError('DeviceBatch.' + what + ": opts.tensor.layout is 'chw' or 'hwc'");
    if (!(channels in TENSOR_CHANNELS)) throw new RangeError('DeviceBatch.' + what + ": opts.tensor.channels is 'rgb', 'bgr' or 'gray'");
    const C = channels === 'gray' ? 1 : 3;
    const coef = function (name, v, dflt) {
      const out = new Float32Array(3);
      if (v === undefined) v = dflt;
      const list = typeof v === 'number' ? new Array(C).fill(v) : Array.from(v || []);
      if (list.length !== C || list.some(function (x) { return typeof x !== 'number'; }))
        throw new TypeError('DeviceBatch.' + what + ': opts.tensor.' + name + ' is a number or ' + C + ' numbers (one per output channel)');
      list.forEach(function (x, c) { out[c] = x; });
      return out;
    };
    return { dtype: TENSOR_DTYPES[dtype], layout: TENSOR_LAYOUTS[layout], channels: TENSOR_CHANNELS[channels], scale: coef('scale', t.scale, 1 / 255), bias: coef('bias', t.bias, 0),
             names: { dtype: dtype, layout: layout, channels: channels }, C: C, esize: dtype === 'f32' ? 4 : 2 };
  };
  /* Prefiltered patches for strong downscales: with opts.prefilter = 1..8 (the largest block factor) the four calls write each patch pixel as
   * the rounded mean of an Nx x Ny block of the unfiltered rule's samples, Nx and Ny chosen per entry on the device from the tracked box
   * (ht_camshift_*_filtered_device: one launch, RGBA8 or — together with opts.tensor — the network's input).  cropResult() / alignResult()
   * then carry `factors`: Int32Array(2 n) [Nx, Ny] per entry (0, 0 for an empty one), from the addon's cropFilterFactors /
   * alignFilterFactors.  Without opts.prefilter nothing changes. */
  const prefilterOf = function (what, o, names) {
    if (o.prefilter === undefined || o.prefilter === null) return 0;
    if (!(Number.isInteger(o.prefilter) && o.prefilter >= 1 && o.prefilter <= 8)) throw new RangeError('DeviceBatch.' + what + ': opts.prefilter is an integer 1..8');
    if (names.some(function (f) { return typeof A[f] !== 'function'; }))
      throw new Error('DeviceBatch.' + what + ': this headtrackr_hip.node has no ' + names.join(' / ') + ' (rebuild it)');
    return o.prefilter;
  };
  const tensorArg = function (t) { return { dtype: t.dtype, layout: t.layout, channels: t.channels, scale: t.scale, bias: t.bias }; };
  const patchBytes = function (prm, t) { return t ? t.C * prm[0] * prm[1] * t.esize : prm[0] * prm[1] * 4; };
  const patchStride = function (prm, t) { return (patchBytes(prm, t) + 3) & ~3; };
  /* the downloaded patches of a tensor call: the elements of all n patches, without the padding behind an odd 16-bit patch */
  const tensorResult = function (last, dev) {
    const t = last.tensor, pb = t.C * last.width * last.height * t.esize, stride = (pb + 3) & ~3, raw = new Uint8Array(last.n * stride);
    A.deviceDownload(ctxs[0], dev, 0, raw);
    let bytes = raw;
    if (stride !== pb) {
      bytes = new Uint8Array(last.n * pb);
      for (let i = 0; i < last.n; i++) bytes.set(raw.subarray(i * stride, i * stride + pb), i * pb);
    }
    const patches = t.esize === 4 ? new Float32Array(bytes.buffer, 0, bytes.length >> 2) : new Uint16Array(bytes.buffer, 0, bytes.length >> 1);
    const shape = t.layout === 0 ? [last.n, t.C, last.height, last.width] : [last.n, last.height, last.width, t.C];
    return { patches: patches, tensor: { dtype: t.names.dtype, layout: t.names.layout, channels: t.names.channels, shape: shape } };
  };
  let cropDev = null, cropBytes = 0, lastCrop = null;
  const needCrop = function (what) {
    if (typeof A.cropPairsDevice !== 'function' || typeof A.cropSourcesDevice !== 'function' || typeof A.cropResult !== 'function')
      throw new Error('DeviceBatch.' + what + ': this headtrackr_hip.node has no cropPairsDevice / cropSourcesDevice / cropResult (rebuild it)');
    if (!trackers) throw new Error('DeviceBatch.' + what + ': no trackers yet (initPairs, initTrackers or detectStep first)');
  };
  const cropParams = function (what, o) {
    if (!o || typeof o !== 'object') throw new TypeError('DeviceBatch.' + what + ': opts is {width, height, margin, square}');
    if (!(Number.isInteger(o.width) && Number.isInteger(o.height) && o.width >= 1 && o.width <= 1024 && o.height >= 1 && o.height <= 1024))
      throw new RangeError('DeviceBatch.' + what + ': opts.width and opts.height are integers 1..1024');
    const margin = o.margin === undefined ? 1 : o.margin;
    if (typeof margin !== 'number' || !(margin >= 0.25 && margin <= 4)) throw new RangeError('DeviceBatch.' + what + ': opts.margin is a number 0.25..4');
    return Int32Array.from([o.width, o.height, Math.round(margin * 256), o.square ? 1 : 0]);
  };
  const cropOut = function (count, prm, t, mf) { /* the patch buffer, grown on demand */
    const need = count * (t ? patchStride(prm, t) : prm[0] * prm[1] * 4);
    if (cropBytes < need) {
      if (cropDev) A.deviceFree(ctxs[0], cropDev); /* waits for the work in flight */
      cropDev = A.deviceAlloc(ctxs[0], need); cropBytes = need;
    }
    lastCrop = { n: count, width: prm[0], height: prm[1], tensor: t || null, prefilter: mf || 0 };
    return cropDev;
  };
  this.cropPairs = function (set, pairs, o) {
    needCrop('cropPairs'); pairList('cropPairs', pairs);
    if (pairs.length > 2 * 65535) throw new RangeError('DeviceBatch.cropPairs: at most 65535 pairs');
    const prm = cropParams('cropPairs', o), mf = prefilterOf('cropPairs', o, ['cropPairsFilteredDevice', 'cropFilterFactors']);
    const t = tensorFormat('cropPairs', o.tensor, [mf ? 'cropPairsFilteredDevice' : 'cropPairsTensorDevice']);
    bind0(set === undefined ? 0 : set);
    if (mf) A.cropPairsFilteredDevice(ctxs[0], pairs, prm, mf, t ? tensorArg(t) : null, cropOut(pairs.length >> 1, prm, t, mf), 0, 0, false);
    else if (t) A.cropPairsTensorDevice(ctxs[0], pairs, prm, tensorArg(t), cropOut(pairs.length >> 1, prm, t), 0, 0, false);
    else A.cropPairsDevice(ctxs[0], pairs, prm, cropOut(pairs.length >> 1, prm), 0, 0, false);
  };
  this.cropFeeds = function (sset, streams, o) {
    needCrop('cropFeeds');
    if (!(streams instanceof Int32Array) || streams.length !== n) throw new TypeError('DeviceBatch.cropFeeds: streams is an Int32Array with one tracker per feed (' + n + ')');
    const prm = cropParams('cropFeeds', o), mf = prefilterOf('cropFeeds', o, ['cropSourcesFilteredDevice', 'cropFilterFactors']);
    const t = tensorFormat('cropFeeds', o.tensor, [mf ? 'cropSourcesFilteredDevice' : 'cropSourcesTensorDevice']), entries = listEntries(sset, o.rects, 'cropFeeds');
    if (mf) A.cropSourcesFilteredDevice(ctxs[0], streams, entries, prm, mf, t ? tensorArg(t) : null, cropOut(n, prm, t, mf), 0, 0, false);
    else if (t) A.cropSourcesTensorDevice(ctxs[0], streams, entries, prm, tensorArg(t), cropOut(n, prm, t), 0, 0, false);
    else A.cropSourcesDevice(ctxs[0], streams, entries, prm, cropOut(n, prm), 0, 0, false);
  };
  this.cropResult = function () {
    if (!lastCrop) throw new Error('DeviceBatch.cropResult: no cropPairs / cropFeeds yet');
    const r = A.cropResult(ctxs[0], lastCrop.n), bytes = lastCrop.n * lastCrop.width * lastCrop.height * 4;
    const res = { n: lastCrop.n, width: lastCrop.width, height: lastCrop.height, records: r.records, ratios: r.ratios };
    if (lastCrop.prefilter) res.factors = A.cropFilterFactors(r.records, lastCrop.width, lastCrop.height, lastCrop.prefilter);
    if (lastCrop.tensor) {
      const tr = tensorResult(lastCrop, cropDev);
      res.patches = tr.patches; res.tensor = tr.tensor;
      return res;
    }
    res.patches = new Uint8Array(bytes);
    A.deviceDownload(ctxs[0], cropDev, 0, res.patches);
    return res;
  };
  /* Angle-aligned face crops (ht_camshift_align_pairs_device / ht_camshift_align_sources_device): the ROTATED box of each tracker — width and
   * height along the blob's axes, turned by its angle as the overlay draws it — sampled upright into opts.width x opts.height RGBA; pixels
   * whose sample centre lies outside the frame are zeros.  Same arguments, options and exclusivity as the crop calls; a patch buffer of their own.
   *   alignPairs(set, pairs, opts) / alignFeeds(sset, streams, opts)
   *   alignResult()                    -> {n, width, height, records: Int32Array(4 n) [code, stream, a12 (the angle in 1/4096 turn), 0],
   *                                    terms: Float64Array(6 n) [cx, cy, ux, uy, vx, vy] (the centre and the patch's two vectors in the source,
   *                                    1/65536 pixel), patches: Uint8Array(n width height 4)} of the LAST align call; waits for it */
  let alignDev = null, alignBytes = 0, lastAlign = null;
  const needAlign = function (what) {
    if (typeof A.alignPairsDevice !== 'function' || typeof A.alignSourcesDevice !== 'function' || typeof A.alignResult !== 'function')
      throw new Error('DeviceBatch.' + what + ': this headtrackr_hip.node has no alignPairsDevice / alignSourcesDevice / alignResult (rebuild it)');
    if (!trackers) throw new Error('DeviceBatch.' + what + ': no trackers yet (initPairs, initTrackers or detectStep first)');
  };
  const alignOut = function (count, prm, t, mf) { /* the patch buffer, grown on demand */
    const need = count * (t ? patchStride(prm, t) : prm[0] * prm[1] * 4);
    if (alignBytes < need) {
      if (alignDev) A.deviceFree(ctxs[0], alignDev); /* waits for the work in flight */
      alignDev = A.deviceAlloc(ctxs[0], need); alignBytes = need;
    }
    lastAlign = { n: count, width: prm[0], height: prm[1], tensor: t || null, prefilter: mf || 0 };
    return alignDev;
  };
  this.alignPairs = function (set, pairs, o) {
    needAlign('alignPairs'); pairList('alignPairs', pairs);
    if (pairs.length > 2 * 65535) throw new RangeError('DeviceBatch.alignPairs: at most 65535 pairs');
    const prm = cropParams('alignPairs', o), mf = prefilterOf('alignPairs', o, ['alignPairsFilteredDevice', 'alignFilterFactors']);
    const t = tensorFormat('alignPairs', o.tensor, [mf ? 'alignPairsFilteredDevice' : 'alignPairsTensorDevice']);
    bind0(set === undefined ? 0 : set);
    if (mf) A.alignPairsFilteredDevice(ctxs[0], pairs, prm, mf, t ? tensorArg(t) : null, alignOut(pairs.length >> 1, prm, t, mf), 0, 0, false);
    else if (t) A.alignPairsTensorDevice(ctxs[0], pairs, prm, tensorArg(t), alignOut(pairs.length >> 1, prm, t), 0, 0, false);
    else A.alignPairsDevice(ctxs[0], pairs, prm, alignOut(pairs.length >> 1, prm), 0, 0, false);
  };
  this.alignFeeds = function (sset, streams, o) {
    needAlign('alignFeeds');
    if (!(streams instanceof Int32Array) || streams.length !== n) throw new TypeError('DeviceBatch.alignFeeds: streams is an Int32Array with one tracker per feed (' + n + ')');
    const prm = cropParams('alignFeeds', o), mf = prefilterOf('alignFeeds', o, ['alignSourcesFilteredDevice', 'alignFilterFactors']);
    const t = tensorFormat('alignFeeds', o.tensor, [mf ? 'alignSourcesFilteredDevice' : 'alignSourcesTensorDevice']), entries = listEntries(sset, o.rects, 'alignFeeds');
    if (mf) A.alignSourcesFilteredDevice(ctxs[0], streams, entries, prm, mf, t ? tensorArg(t) : null, alignOut(n, prm, t, mf), 0, 0, false);
    else if (t) A.alignSourcesTensorDevice(ctxs[0], streams, entries, prm, tensorArg(t), alignOut(n, prm, t), 0, 0, false);
    else A.alignSourcesDevice(ctxs[0], streams, entries, prm, alignOut(n, prm), 0, 0, false);
  };
  this.alignResult = function () {
    if (!lastAlign) throw new Error('DeviceBatch.alignResult: no alignPairs / alignFeeds yet');
    const r = A.alignResult(ctxs[0], lastAlign.n), bytes = lastAlign.n * lastAlign.width * lastAlign.height * 4;
    const res = { n: lastAlign.n, width: lastAlign.width, height: lastAlign.height, records: r.records, terms: r.terms };
    if (lastAlign.prefilter) res.factors = A.alignFilterFactors(r.records, r.terms, lastAlign.width, lastAlign.height, lastAlign.prefilter);
    if (lastAlign.tensor) {
      const tr = tensorResult(lastAlign, alignDev);
      res.patches = tr.patches; res.tensor = tr.tensor;
      return res;
    }
    res.patches = new Uint8Array(bytes);
    A.deviceDownload(ctxs[0], alignDev, 0, res.patches);
    return res;
  };
  this.graphLaunches = function () { return ctxs.reduce(function (s, c) { return s + A.graphLaunches(c); }, 0); };
  /* the frame buffer is shared by all `depth` contexts: the others go first (ht_device_free refuses while they have it bound) */
  this.destroy = function () { for (let i = ctxs.length - 1; i >= 1; i--) A.destroy(ctxs[i]); if (sdev) A.deviceFree(ctxs[0], sdev); if (feeds) feeds.forEach(function (f) { A.deviceFree(ctxs[0], f.dev); }); if (cropDev) A.deviceFree(ctxs[0], cropDev); if (alignDev) A.deviceFree(ctxs[0], alignDev); A.deviceFree(ctxs[0], dev); A.destroy(ctxs[0]); ctxs.length = 0; };
};

/* ---- whitebalance ----------------------------------------------------------------------------------------------------- */

headtrackr.getWhitebalance = function (canvas) { /* whitebalance.js:5-30 */
  const img = canvas.getContext('2d').getImageData(0, 0, canvas.width, canvas.height);
  if (!(img.width > 0 && img.height > 0)) return NaN; /* 0/0 in the reference */
  const c = contextFor(headtrackr.cascade, 5);
  /* announce the size like every other entry point: a frame of another size would make the addon re-build the geometry on its own, with
   * level sizes from libm instead of V8's, behind the back of the cache in `c` (found by tests/js/parity_cpu.js) */
  ensureGeometry(c, img.width, img.height, 1, headtrackr.cascade, 5);
  c.boundImg = null;
  return addon().whitebalance(c.handle, img.data, 1, img.width, img.height)[0];
};

/* ---- camshift ----------------------------------------------------------------------------------------------------------- */

headtrackr.camshift = {};

headtrackr.camshift.Histogram = function (imgdata) { /* camshift.js:49-72 (host-side; used by the debug getters) */
  this.size = 4096;
  const bins = new Uint32Array(4096);
  for (let x = 0, il = imgdata.length; x < il; x += 4) bins[256 * (imgdata[x] >> 4) + 16 * (imgdata[x + 1] >> 4) + (imgdata[x + 2] >> 4)] += 1;
  this.getBin = function (index) { return bins[index]; };
};

headtrackr.camshift.Moments = function (data, x, y, w, h, second) { /* camshift.js:79-120 (host-side, for API completeness) */
  this.m00 = 0; this.m01 = 0; this.m10 = 0; this.m11 = 0; this.m02 = 0; this.m20 = 0;
  for (let i = x; i < w; i++) {
    const col = data[i], vx = i - x;
    for (let j = y; j < h; j++) {
      const val = col[j], vy = j - y;
      this.m00 += val; this.m01 += vy * val; this.m10 += vx * val;
      if (second) { this.m11 += vx * vy * val; this.m02 += vy * vy * val; this.m20 += vx * vx * val; }
    }
  }
  this.invM00 = 1 / this.m00;
  this.xc = this.m10 * this.invM00;
  this.yc = this.m01 * this.invM00;
  this.mu00 = this.m00; this.mu01 = 0; this.mu10 = 0;
  if (second) {
    this.mu20 = this.m20 - this.m10 * this.xc;
    this.mu02 = this.m02 - this.m01 * this.yc;
    this.mu11 = this.m11 - this.m01 * this.xc;
  }
};

headtrackr.camshift.Rectangle = function (x, y, w, h) { /* camshift.js:127-141 */
  this.x = x; this.y = y; this.width = w; this.height = h;
  this.clone = function () { return new headtrackr.camshift.Rectangle(this.x, this.y, this.width, this.height); };
};

headtrackr.camshift.TrackObj = function () { /* camshift.js:362-378 */
  this.height = 0; this.width = 0; this.angle = 0; this.x = 0; this.y = 0;
  this.clone = function () {
    const c = new headtrackr.camshift.TrackObj();
    c.height = this.height; c.width = this.width; c.angle = this.angle; c.x = this.x; c.y = this.y;
    return c;
  };
};

/* every camshift.Tracker owns one device-side stream slot of a shared context */
const csPool = { ctx: null, next: 0, free: [], reserved: 0, pairSchedule: 'workgroup' };
function csSlot() {
  if (!csPool.ctx) csPool.ctx = contextFor(headtrackr.cascade, 5, undefined, pairScheduleOptions(csPool.pairSchedule, 'headtrackr.camshift') || undefined);
  const slot = csPool.free.length ? csPool.free.pop() : csPool.next++;
  if (csPool.next > csPool.reserved) { /* grow geometrically: a reservation re-allocates and copies every tracker's state */
    csPool.reserved = Math.max(csPool.next, 2 * csPool.reserved, 4);
    addon().camshiftReserve(csPool.ctx.handle, csPool.reserved);
  }
  return slot;
}
headtrackr.camshift._pool = csPool; /* exposed for tests */
/* headtrackr.camshift.pairSchedule = 'workgroup' (default) | 'cluster': the schedule of camshift.MultiTracker's pair calls (and the option of
 * the context every camshift.Tracker shares with it).  Read when the pool's context is created, i.e. by the first Tracker / MultiTracker:
 * set it BEFORE that; afterwards a change throws. */
Object.defineProperty(headtrackr.camshift, 'pairSchedule', {
  enumerable: true,
  get: function () { return csPool.pairSchedule; },
  set: function (v) {
    pairScheduleOptions(v, 'headtrackr.camshift'); /* RangeError for anything else */
    if (v === csPool.pairSchedule) return;
    if (csPool.ctx) throw new Error('headtrackr.camshift.pairSchedule must be set before the first camshift.Tracker / MultiTracker is created (the camshift context exists already)');
    csPool.pairSchedule = v;
  }
});

/* getPdf() on the host (camshift.js:198-211, 314-353): `last` through the model of rect `mr` on `mframe` (both ImageData) */
function hostPdf(last, mframe, mr) {
  const w = last.width, h = last.height, d = last.data;
  const mw = mframe.width, mh = mframe.height, md = mframe.data;
  const model = new Uint32Array(4096);
  for (let y = mr.y; y < mr.y + mr.height; y++) {
    for (let x = mr.x; x < mr.x + mr.width; x++) {
      if (x >= 0 && x < mw && y >= 0 && y < mh) {
        const p = (y * mw + x) * 4;
        model[256 * (md[p] >> 4) + 16 * (md[p + 1] >> 4) + (md[p + 2] >> 4)]++;
      } else model[0]++;
    }
  }
  const cur = new headtrackr.camshift.Histogram(d);
  const weights = new Float64Array(4096);
  for (let i = 0; i < 4096; i++) weights[i] = cur.getBin(i) !== 0 ? Math.min(model[i] / cur.getBin(i), 1) : 0;
  const data = [];
  for (let x = 0; x < w; x++) {
    const col = [];
    for (let y = 0; y < h; y++) {
      const p = (y * w + x) * 4;
      col.push(weights[256 * (d[p] >> 4) + 16 * (d[p + 1] >> 4) + (d[p + 2] >> 4)]);
    }
    data[x] = col;
  }
  return data;
}
/* getBackProjectionImg() from a pdf (camshift.js:177-196) */
function pdfToImg(ctx2d, pdf, w, h) {
  const img = ctx2d.createImageData(w, h), out = img.data;
  for (let x = 0; x < w; x++) {
    for (let y = 0; y < h; y++) {
      const v = Math.floor(255 * pdf[x][y]), p = (y * w + x) * 4;
      out[p] = v; out[p + 1] = v; out[p + 2] = v; out[p + 3] = 255;
    }
  }
  return img;
}

headtrackr.camshift.Tracker = function (params) { /* camshift.js:148-354 */
  if (params === undefined) params = {};
  if (params.calcAngles === undefined) params.calcAngles = true;
  const slot = csSlot();
  let searchWindow = null, trackObj = null, lastFrame = null, modelRect = null, modelFrame = null, canvasCtx = null;

  this.getSearchWindow = function () { return searchWindow.clone(); };
  this.getTrackObj = function () { return trackObj.clone(); };

  /* the work of initTracker / track on an ImageData; the frame is uploaded unless the caller already has (bindFrame) */
  this._initImg = function (img, trackedArea, ctx2d) {
    canvasCtx = ctx2d;
    const rect = new Int32Array([trackedArea.x, trackedArea.y, trackedArea.width, trackedArea.height]);
    if (img.width > 0 && img.height > 0) {
      bindFrame(csPool.ctx, img, headtrackr.cascade, 5);
      addon().camshiftInitBound(csPool.ctx.handle, 1, slot, rect);
    }
    modelFrame = img; modelRect = trackedArea.clone();
    searchWindow = trackedArea.clone();
    trackObj = new headtrackr.camshift.TrackObj();
  };
  this._trackImg = function (img) {
    if (img.width === 0 || img.height === 0) return;
    lastFrame = img;
    bindFrame(csPool.ctx, img, headtrackr.cascade, 5);
    const r = addon().camshiftTrackBound(csPool.ctx.handle, 1, slot, params.calcAngles ? 1 : 0, true);
    trackObj.x = r[0]; trackObj.y = r[1]; trackObj.width = r[2]; trackObj.height = r[3]; trackObj.angle = r[4];
    searchWindow.x = r[5]; searchWindow.y = r[6]; searchWindow.width = r[7]; searchWindow.height = r[8];
  };

  this.initTracker = function (canvas, trackedArea) { /* camshift.js:198-211 */
    const ctx2d = canvas.getContext('2d');
    try { this._initImg(ctx2d.getImageData(0, 0, canvas.width, canvas.height), trackedArea, ctx2d); } finally { unbindFrames(); }
  };

  this.track = function (canvas) { /* camshift.js:213-259 */
    try { this._trackImg(canvas.getContext('2d').getImageData(0, 0, canvas.width, canvas.height)); } finally { unbindFrames(); }
  };

  /* debug getters (camshift.js:172-196, 314-353).  getPdf's result is an array of W arrays of boxed numbers — a W x H JavaScript loop
   * whatever the source —, so it is rebuilt here from the last frame; getBackProjectionImg's bytes come from the device (below) */
  this.getPdf = function () {
    if (!lastFrame || !modelFrame) return undefined;
    return hostPdf(lastFrame, modelFrame, modelRect);
  };

  this.getBackProjectionImg = function () {
    /* device route (ht_camshift_backproject): the last frame through this tracker's model.  Inside facetrackr's detectCS the frame is
     * still bound from _trackImg and bindFrame is a no-op; a stand-alone call uploads it again and drops the marker like every public
     * entry point.  An addon without the entry point (the CPU test doubles) takes the host loop below. */
    if (lastFrame && modelFrame && modelFrame.width > 0 && modelFrame.height > 0 && typeof addon().camshiftBackProject === 'function') {
      const mine = csPool.ctx.boundImg !== lastFrame;
      try {
        bindFrame(csPool.ctx, lastFrame, headtrackr.cascade, 5);
        const img = canvasCtx.createImageData(lastFrame.width, lastFrame.height);
        img.data.set(addon().camshiftBackProject(csPool.ctx.handle, 1, slot, addon().BP_RGBA8));
        return img;
      } finally { if (mine) unbindFrames(); }
    }
    return pdfToImg(canvasCtx, this.getPdf(), lastFrame.width, lastFrame.height);
  };

  /* not in the reference: returns the device slot (idempotent).  facetrackr.Tracker.release() calls it when the facade
   * replaces a tracker on "redetecting" / stop(), so a long-running feed that loses its face keeps one slot. */
  let released = false;
  this.release = function () { if (!released) { released = true; csPool.free.push(slot); } };
};

/* not in the reference: M camshift trackers on ONE canvas — what a page does with one camshift.Tracker per detected face — with one
 * upload and one device call per frame (ht_camshift_track_pairs, every pair on frame 0: the frame's histogram is computed once, not M
 * times).  Results equal M camshift.Tracker instances on that canvas; the slots come from the same pool.
 *   initTracker(canvas, rects)   rects: array of camshift.Rectangle (or {x, y, width, height}), one tracker each (camshift.js:198-211)
 *   track(canvas)                one track() of every tracker (camshift.js:213-353)
 *   getTrackObj(i) / getSearchWindow(i) / release()
 *   getBackProjectionImg(i)      ImageData: the last tracked canvas through tracker i's model (camshift.js:177-196)
 *   getBackProjectionImgs()      all of them, in ONE device call (ht_camshift_backproject_pairs: the canvas is read once per 4 trackers)
 *   getPdf(i)                    the reference's [x][y] arrays (camshift.js:172-175), rebuilt from the device's binary64 output
 * The getters re-bind the last canvas and unbind it afterwards, like camshift.Tracker.getBackProjectionImg; with an addon that lacks
 * camshiftBackProjectPairs they run the host loop, with the same result.  Before the first track() they return undefined. */
headtrackr.camshift.MultiTracker = function (params) {
  if (params === undefined) params = {};
  if (params.calcAngles === undefined) params.calcAngles = true;
  let slots = [], pairs = null, windows = [], objs = [];
  let lastFrame = null, modelFrame = null, modelRects = [], canvasCtx = null;
  const needPairs = function () {
    if (typeof addon().camshiftInitPairs !== 'function' || typeof addon().camshiftTrackPairs !== 'function')
      throw new Error('camshift.MultiTracker: this headtrackr_hip.node has no camshiftInitPairs / camshiftTrackPairs (rebuild it)');
  };
  this.count = function () { return slots.length; };
  this.getSearchWindow = function (i) { return windows[i].clone(); };
  this.getTrackObj = function (i) { return objs[i].clone(); };
  this.release = function () {
    slots.forEach(function (s) { csPool.free.push(s); });
    slots = []; pairs = null; windows = []; objs = []; lastFrame = null; modelFrame = null; modelRects = []; canvasCtx = null;
  };
  /* the bytes of the device call for trackers [first, first + m): Uint8Array(4 m w h) or Float64Array(m w h) */
  const deviceBp = function (first, m, kind) {
    try {
      bindFrame(csPool.ctx, lastFrame, headtrackr.cascade, 5);
      return addon().camshiftBackProjectPairs(csPool.ctx.handle, pairs.subarray(2 * first, 2 * (first + m)), kind);
    } finally { unbindFrames(); }
  };
  const onDevice = function () { return typeof addon().camshiftBackProjectPairs === 'function' && modelFrame.width > 0 && modelFrame.height > 0; };
  const imgsOf = function (first, m) {
    if (!lastFrame || !modelFrame) return undefined;
    const w = lastFrame.width, h = lastFrame.height, out = [];
    if (onDevice()) {
      const bytes = deviceBp(first, m, addon().BP_RGBA8);
      for (let i = 0; i < m; i++) {
        const img = canvasCtx.createImageData(w, h);
        img.data.set(bytes.subarray(4 * w * h * i, 4 * w * h * (i + 1)));
        out.push(img);
      }
    } else {
      for (let i = first; i < first + m; i++) out.push(pdfToImg(canvasCtx, hostPdf(lastFrame, modelFrame, modelRects[i]), w, h));
    }
    return out;
  };
  const tracker = function (what, i) {
    if (!(i >= 0 && i < slots.length && Math.floor(i) === i)) throw new RangeError('camshift.MultiTracker.' + what + '(i): i is 0 .. count() - 1');
  };
  this.getBackProjectionImg = function (i) { tracker('getBackProjectionImg', i); const r = imgsOf(i, 1); return r && r[0]; };
  this.getBackProjectionImgs = function () { return imgsOf(0, slots.length); };
  this.getPdf = function (i) {
    tracker('getPdf', i);
    if (!lastFrame || !modelFrame) return undefined;
    if (!onDevice()) return hostPdf(lastFrame, modelFrame, modelRects[i]);
    const w = lastFrame.width, h = lastFrame.height, v = deviceBp(i, 1, addon().BP_F64), data = [];
    for (let x = 0; x < w; x++) {
      const col = [];
      for (let y = 0; y < h; y++) col.push(v[y * w + x]);
      data[x] = col;
    }
    return data;
  };
  this.initTracker = function (canvas, rects) {
    needPairs();
    if (!rects || !rects.length) throw new TypeError('camshift.MultiTracker.initTracker(canvas, rects): at least one rect');
    this.release();
    for (let i = 0; i < rects.length; i++) slots.push(csSlot());
    pairs = new Int32Array(2 * rects.length);
    const rc = new Int32Array(4 * rects.length);
    rects.forEach(function (r, i) {
      pairs[2 * i] = slots[i]; pairs[2 * i + 1] = 0;
      rc[4 * i] = r.x; rc[4 * i + 1] = r.y; rc[4 * i + 2] = r.width; rc[4 * i + 3] = r.height;
      windows.push(new headtrackr.camshift.Rectangle(r.x, r.y, r.width, r.height));
      modelRects.push(new headtrackr.camshift.Rectangle(r.x, r.y, r.width, r.height));
      objs.push(new headtrackr.camshift.TrackObj());
    });
    canvasCtx = canvas.getContext('2d');
    const img = canvasCtx.getImageData(0, 0, canvas.width, canvas.height);
    modelFrame = img;
    if (!(img.width > 0 && img.height > 0)) return;
    try {
      bindFrame(csPool.ctx, img, headtrackr.cascade, 5);
      addon().camshiftInitPairs(csPool.ctx.handle, pairs, rc);
    } finally { unbindFrames(); }
  };
  this.track = function (canvas) {
    if (!pairs) throw new Error('camshift.MultiTracker.track: initTracker first');
    const img = canvas.getContext('2d').getImageData(0, 0, canvas.width, canvas.height);
    if (img.width === 0 || img.height === 0) return; /* camshift.js:219 */
    lastFrame = img;
    let r;
    try {
      bindFrame(csPool.ctx, img, headtrackr.cascade, 5);
      r = addon().camshiftTrackPairs(csPool.ctx.handle, pairs, params.calcAngles ? 1 : 0, true);
    } finally { unbindFrames(); }
    for (let i = 0; i < slots.length; i++) {
      const o = objs[i], w = windows[i], b = 9 * i;
      o.x = r[b]; o.y = r[b + 1]; o.width = r[b + 2]; o.height = r[b + 3]; o.angle = r[b + 4];
      w.x = r[b + 5]; w.y = r[b + 6]; w.width = r[b + 7]; w.height = r[b + 8];
    }
  };
};

/* ---- facetrackr ------------------------------------------------------------------------------------------------------------ */

headtrackr.facetrackr = {};

headtrackr.facetrackr.TrackObj = function () { /* facetrackr.js:233-255 */
  this.height = 0; this.width = 0; this.angle = 0; this.x = 0; this.y = 0;
  this.confidence = -10000; this.detection = ''; this.time = 0;
  this.clone = function () {
    const c = new headtrackr.facetrackr.TrackObj();
    c.height = this.height; c.width = this.width; c.angle = this.angle; c.x = this.x; c.y = this.y;
    c.confidence = this.confidence; c.detection = this.detection; c.time = this.time;
    return c;
  };
};

function now() { return (new Date()).getTime(); }

headtrackr.facetrackr.Tracker = function (params) { /* facetrackr.js:37-228 */
  if (!params) params = {};
  if (params.sendEvents === undefined) params.sendEvents = true;
  if (params.whitebalancing === undefined) params.whitebalancing = true;
  if (params.debug === undefined || params.debug.tagName !== 'CANVAS') params.debug = false;
  if (params.calcAngles === undefined) params.calcAngles = false;
  let state = params.whitebalancing ? 'WB' : 'VJ';
  let input = null, current = null, cs = null;
  const confidenceThreshold = -10; /* facetrackr.js:57 */
  const wbWindow = [], wbLength = 15; /* facetrackr.js:58-59 */

  this.init = function (inputcanvas) {
    input = inputcanvas;
    if (cs) cs.release(); /* a second init() reuses nothing of the first (facetrackr.js:61-65 builds a new camshift.Tracker) */
    cs = new headtrackr.camshift.Tracker({ calcAngles: params.calcAngles });
  };

  function detectVJ(img) { /* facetrackr.js:133-182; the canvas copy + grayscale are fused into the device path */
    const start = now();
    const comp = (img.width > 0 && img.height > 0) ? detectBoundImg(img, headtrackr.cascade, 5, 1) : [];
    const diff = now() - start;
    let best;
    for (let i = 0; i < comp.length; i++) if (best === undefined || comp[i].confidence > best.confidence) best = comp[i];
    const result = new headtrackr.facetrackr.TrackObj();
    if (best !== undefined) {
      result.width = best.width; result.height = best.height; result.x = best.x; result.y = best.y; result.confidence = best.confidence;
    }
    result.time = diff;
    result.detection = 'VJ';
    return result;
  }

  function detectCS(img) { /* facetrackr.js:185-217 */
    const start = now();
    cs._trackImg(img);
    const r = cs.getTrackObj();
    if (params.debug) params.debug.getContext('2d').putImageData(cs.getBackProjectionImg(), 0, 0);
    const result = new headtrackr.facetrackr.TrackObj();
    result.width = r.width; result.height = r.height; result.x = r.x; result.y = r.y; result.angle = r.angle;
    result.confidence = 1;
    result.time = now() - start;
    result.detection = 'CS';
    return result;
  }

  function checkWB(img) { /* facetrackr.js:220-227 */
    const result = new headtrackr.facetrackr.TrackObj();
    if (img.width > 0 && img.height > 0) {
      const c = contextFor(headtrackr.cascade, 5);
      bindFrame(c, img, headtrackr.cascade, 5);
      result.wb = addon().whitebalanceBound(c.handle, 1)[0];
    } else result.wb = NaN; /* 0/0 in the reference */
    result.detection = 'WB';
    return result;
  }

  this.track = function () { /* facetrackr.js:67-126 */
    /* the frame is read from the canvas and uploaded ONCE per call; whatever runs on it (whitebalance, detection, initTracker,
     * track) shares that copy — the reference calls getImageData in each of them (whitebalance.js:12, facetrackr.js:143-149,
     * camshift.js:206,218), here that would be one PCIe transfer each */
    const ctx2d = input.getContext('2d');
    const img = ctx2d.getImageData(0, 0, input.width, input.height);
    let result;
    try {
      if (state === 'WB') result = checkWB(img);
      else if (state === 'VJ') result = detectVJ(img);
      else result = detectCS(img);
      if (result.detection === 'VJ' && result.confidence > confidenceThreshold) { /* facetrackr.js:97-108 */
        state = 'CS';
        cs._initImg(img, new headtrackr.camshift.Rectangle(Math.floor(result.x), Math.floor(result.y),
          Math.floor(result.width), Math.floor(result.height)), ctx2d);
      }
    } finally { unbindFrames(); } /* the uploaded copy is shared within this call only */

    if (result.detection === 'WB') { /* facetrackr.js:79-95 */
      if (wbWindow.length >= wbLength) wbWindow.pop();
      wbWindow.unshift(result.wb);
      if (wbWindow.length === wbLength && Math.max.apply(null, wbWindow) - Math.min.apply(null, wbWindow) < 2) state = 'VJ';
    }
    current = result;
    if (result.detection === 'CS' && params.sendEvents) { /* facetrackr.js:112-125 */
      const hasDoc = typeof document !== 'undefined' && document.createEvent;
      const evt = hasDoc ? document.createEvent('Event') : { type: 'facetrackingEvent' };
      if (hasDoc) evt.initEvent('facetrackingEvent', true, true);
      evt.height = result.height; evt.width = result.width; evt.angle = result.angle; evt.x = result.x; evt.y = result.y;
      evt.confidence = result.confidence; evt.detection = result.detection; evt.time = result.time;
      if (hasDoc) document.dispatchEvent(evt);
      if (params.onEvent) params.onEvent('facetrackingEvent', evt); /* Node hosts without a DOM */
    }
  };

  this.getTrackingObject = function () { return current.clone(); };

  this.release = function () { if (cs) { cs.release(); cs = null; } }; /* not in the reference: frees the camshift device slot */
};

require('./tracker.js')(headtrackr); /* Smoother, headposition, Tracker facade (host post-processing) */

module.exports = headtrackr;
